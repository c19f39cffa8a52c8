"""CPU tests of include/ptr_deform_device.h: the exported surface, what ptr_scene_upload_deformable refuses, the vertex adjacency the new
flag keeps against the numpy restatement (tests/deform_device_ref.py), that the preparation without the flag is what it was, and the
stand-alone sanitizer program.  No GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deform_device_ref as ref
import deform_device_scenes as dds
import deform_scenes as dsc
import traversal_scenes as ts

pt = ts.pt
ROOT = ts.ROOT
VECTORS = os.path.join(ts.GOLDEN, "vectors")


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_device_deform_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "ptr_deform_device.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, 0 if args.strip() in ("", "void") else args.count(",") + 1)
             for kind, name, args in re.findall(r"\b(int|uint32_t)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {"ptr_scene_upload_deformable": ("int", 6), "ptr_scene_set_mesh_vertices_device": ("int", 7), "ptr_debug_vertex_adjacency": ("int", 7)}
    assert set(found) == set(pt.DEFORM_DEVICE_SYMBOLS)
    lib = pt.load_library()
    for name, (kind, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is C.c_int, name
    others = [pt.ABI_SYMBOLS, pt.DEBUG_SYMBOLS, pt.POST_SYMBOLS, pt.STATS_SYMBOLS, pt.ADAPTIVE_SYMBOLS, pt.MULTI_SYMBOLS, pt.FRAME_SYMBOLS,
              pt.MULTI_FRAME_SYMBOLS, pt.DYNAMIC_SYMBOLS, pt.DEFORM_SYMBOLS, pt.BACKGROUND_SYMBOLS]
    assert not set(pt.DEFORM_DEVICE_SYMBOLS) & set().union(*others)
    # the ctypes mirror has the header's size and offsets, the flag the header's value
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_deform_device.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(PtrMeshVerticesDevice), offsetof(PtrMeshVerticesDevice, meshIndex), offsetof(PtrMeshVerticesDevice, vertexCount), "
                   "offsetof(PtrMeshVerticesDevice, positions), offsetof(PtrMeshVerticesDevice, normals), offsetof(PtrMeshVerticesDevice, tangents), "
                   "(int)PTR_DYNAMIC_VERTEX_NORMALS); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    mv = pt.PtrMeshVerticesDevice
    assert got == [C.sizeof(mv), mv.meshIndex.offset, mv.vertexCount.offset, mv.positions.offset, mv.normals.offset, mv.tangents.offset,
                   pt.PTR_DYNAMIC_VERTEX_NORMALS] == [32, 0, 4, 8, 16, 24, 4]
    assert C.sizeof(mv) == C.sizeof(pt.PtrMeshVertices), "the two lists share their validation: same members"
    assert not pt.PTR_DYNAMIC_VERTEX_NORMALS & (pt.PTR_DYNAMIC_DEFORMABLE | pt.PTR_DYNAMIC_PRIMITIVES)


def test_what_the_upload_and_the_entry_points_refuse_without_a_device():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    out = C.c_void_p()
    desc = pt.PtrSceneDesc()
    assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, 8, C.byref(out), err, len(err)) == 1
    assert err.value == b"ptr_scene_upload_deformable: unknown flag"
    assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, 15, C.byref(out), err, len(err)) == 1 and b"unknown flag" in err.value
    for flags in (4, 6):
        assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, flags, C.byref(out), err, len(err)) == 1
        assert err.value == b"ptr_scene_upload_deformable: PTR_DYNAMIC_VERTEX_NORMALS needs PTR_DYNAMIC_DEFORMABLE"
    assert lib.ptr_scene_upload_deformable(None, 0, 5, C.byref(out), err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, 5, None, err, len(err)) == 1 and b"null argument" in err.value
    # the older entry point keeps refusing the new bit
    assert lib.ptr_scene_upload_dynamic_ex(C.byref(desc), 0, 5, C.byref(out), err, len(err)) == 1 and b"unknown flag" in err.value
    assert lib.ptr_scene_set_mesh_vertices_device(None, None, 0, None, None, err, len(err)) == 1 and b"null argument" in err.value
    n = C.c_uint64(0)
    assert lib.ptr_debug_vertex_adjacency(None, 0, None, 0, C.byref(n), err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_debug_vertex_adjacency(C.byref(desc), 0, None, 0, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_debug_vertex_adjacency(C.byref(desc), 0, None, 0, C.byref(n), err, len(err)) == 1 and b"out of range" in err.value
    if pt.device_count() < 1:
        for flags in (0, 3, 5, 7):
            assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, flags, C.byref(out), err, len(err)) == 2
            assert err.value.decode().startswith("ptr_scene_upload_deformable: no HIP device") and not out.value
    assert not out.value


# --------------------------------------------------------------------------- the adjacency
def adjacency_scenes(tmp):
    yield "textured", pt.HostScene.load(os.path.join(ts.GOLDEN, "textured.scene"), ts.GOLDEN)
    yield "triangle", ts.scene_f(tmp, "triangle")
    yield "coincident", ts.scene_f(tmp, "coincident")
    for key in ("fan", "odd", "cancel", "strip1", "strip257"):
        yield key, dds.remeshed(tmp, key)


def test_vertex_adjacency_equals_the_reference(tmp_path):
    triangles = {}
    for key, host in adjacency_scenes(tmp_path):
        corners = pt.debug_dynamic_tables(host.desc, ["meshCorners", "meshTriOffsets"])
        triangles[key] = 0
        for m in range(host.desc.meshCount):
            mesh = host.desc.meshes[m]
            idx = np.ctypeslib.as_array(mesh.indices, (mesh.indexCount // 3, 3)).copy()
            offsets, entries = pt.debug_vertex_adjacency(host.desc, m)
            want_offsets, want_entries = ref.adjacency(idx, mesh.vertexCount)
            assert np.array_equal(offsets, want_offsets) and np.array_equal(entries, want_entries), (key, m)
            # and against the description itself: every entry of vertex v is a triangle that names v, once per corner, in ascending order;
            # the triangle's indices are where the kernel finds them, in this mesh's part of the corner table
            first = corners["meshTriOffsets"][m]
            table = corners["meshCorners"][first:corners["meshTriOffsets"][m + 1]]
            assert np.array_equal(table, idx), (key, m)
            assert len(offsets) == mesh.vertexCount + 1 and offsets[0] == 0 and offsets[-1] == len(entries) == idx.size
            for v in range(mesh.vertexCount):
                row = entries[offsets[v]:offsets[v + 1]]
                assert (np.diff(row.astype(np.int64)) >= 0).all(), (key, m, v)
                assert np.array_equal(np.bincount(row, minlength=len(idx)), (idx == v).sum(axis=1)), (key, m, v)
            triangles[key] += len(idx)
    assert triangles["textured"] > 257 and triangles["strip257"] == 255 and triangles["triangle"] == 1 and triangles["coincident"] == 9
    # what each of the built meshes is there for
    fan = dds.remeshed(tmp_path, "fan")
    offsets, _ = pt.debug_vertex_adjacency(fan.desc, 0)
    assert offsets[1] - offsets[0] == 70
    odd = dds.remeshed(tmp_path, "odd")
    offsets, entries = pt.debug_vertex_adjacency(odd.desc, 0)
    assert offsets[6] == offsets[5], "vertex 5 is unreferenced"
    assert list(entries[offsets[1]:offsets[2]]) == [0, 1, 2, 2] and list(entries[offsets[3]:offsets[4]]) == [1, 3, 3, 3]
    one = dds.remeshed(tmp_path, "strip1")
    assert [list(a) for a in pt.debug_vertex_adjacency(one.desc, 0)] == [[0, 3], [0, 0, 0]]


def test_adjacency_of_a_mesh_without_triangles(tmp_path):
    bare = dsc.Changed(ts.scene_f(tmp_path, "triangle"))
    bare._meshes[0].indexCount = 0
    offsets, entries = pt.debug_vertex_adjacency(bare.desc, 0)
    assert list(offsets) == [0, 0, 0, 0] and len(entries) == 0


def test_reference_normals_on_cases_worked_by_hand():
    # a right triangle in z = 0, counter-clockwise: every vertex gets +z; cross = (0, 0, 2 * 3)
    n = ref.normals([(0, 0, 0), (2, 0, 0), (0, 3, 0)], [(0, 1, 2)])
    assert n.dtype == np.float32 and np.array_equal(n, np.array([[0, 0, 1]] * 3, np.float32))
    # both windings cancel to +0, an unreferenced vertex is zero, a vertex named three times sums three zero cross products
    verts, faces = dds.cancel()
    n = ref.normals(verts, faces)
    assert np.array_equal(n[0].view(np.uint32), np.zeros(3, np.uint32)), "+0, not -0"
    assert np.linalg.norm(n[3]) == pytest.approx(1.0, abs=1e-6)
    verts, faces = dds.odd()
    assert np.array_equal(ref.normals(verts, faces)[5], np.zeros(3, np.float32))
    assert np.array_equal(ref.normals(*dds.strip(1)), np.zeros((1, 3), np.float32))
    # area weighting: two triangles at vertex 0, areas 1/2 and 4 in planes z = 0 and x = 0: the sum is (8, 0, 1) / sqrt(65)
    n = ref.normals([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 4), (0, 2, 0)], [(0, 1, 2), (0, 4, 3)])
    want = np.array([8.0, 0.0, 1.0], np.float32) * (np.float32(1.0) / np.sqrt(np.float32(65.0)))
    assert np.array_equal(n[0], want)
    # positions of 3e38: the edges overflow and the normal is not finite
    big = ref.normals(np.array([(3e38, 0, 0), (-3e38, 0, 0), (0, 3e38, 0)], np.float32), [(0, 1, 2)])
    assert not np.isfinite(big).all()


# --------------------------------------------------------------------------- the preparation without the flag did not change
OLD_TABLES = [k for k, v in pt.DYNAMIC_TABLES.items() if v[0] <= 12 and k != "info"]


def test_preparation_with_the_old_flags_is_what_the_commit_before_produced():
    """ptr_scene_upload_dynamic, ptr_scene_upload_dynamic_ex and ptr_scene_upload_deformable go through one function and one preparation;
    ptr_debug_dynamic_tables shows that preparation for flags 3.  tests/golden/vectors/dynamic_tables_parent.json holds size and SHA-256 of
    every table of scene A from before ptr_deform.h existed (test_dynamic_deform_host.py).  The same comparison through both upload calls
    on the device is test_gpu_deform_device.py::test_old_flags_upload_the_same_scene_through_either_call."""
    want = json.load(open(os.path.join(VECTORS, "dynamic_tables_parent.json")))["A"]
    host = ts.scene_a()
    got = pt.debug_dynamic_tables(host.desc, OLD_TABLES + ["info"])
    assert got["info"] == want["info"]
    for name in OLD_TABLES:
        a = np.ascontiguousarray(got[name])
        assert a.nbytes == want[name]["bytes"] and hashlib.sha256(a.tobytes()).hexdigest() == want[name]["sha256"], name


# --------------------------------------------------------------------------- the sanitizer program
def test_the_stand_alone_host_check_builds_and_runs_clean(tmp_path):
    """tools/deform_device_host_check.cpp with -fsanitize=address,undefined: a stand-alone program on the CPU with its own main and the
    sanitizers' runtimes linked in."""
    csrc = os.path.join(ROOT, "metal-pathtracer-arm64_amd", "csrc")
    exe = tmp_path / "deform_device_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(csrc, "host"), "-I", os.path.join(csrc, "kernels"), os.path.join(ROOT, "tools", "deform_device_host_check.cpp"),
                    os.path.join(csrc, "host", "scene_geometry.cpp"), os.path.join(csrc, "host", "bvh_builder.cpp"), os.path.join(csrc, "host", "knobs.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    lines = res.stdout.strip().split("\n")
    assert lines[0] == "0 triangles: ok" and lines[-2] == "20000 triangles: ok" and lines[-1] == "single calls: ok" and len(lines) == 12
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout
