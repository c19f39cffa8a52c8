"""CPU tests of include/ptr_deform.h: the exported surface, the tables the new upload flags keep, that the preparation of a dynamic scene
is what it was, and that the row writers the update calls share with the upload produce the upload's rows.  No GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deform_scenes as dsc
import traversal_scenes as ts

pt = ts.pt
ROOT = ts.ROOT
VECTORS = os.path.join(ts.GOLDEN, "vectors")


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_deform_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "ptr_deform.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, 0 if args.strip() in ("", "void") else args.count(",") + 1)
             for kind, name, args in re.findall(r"\b(int|uint32_t)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {"ptr_scene_upload_dynamic_ex": ("int", 6), "ptr_scene_dynamic_flags": ("uint32_t", 1), "ptr_scene_set_mesh_vertices": ("int", 7),
                     "ptr_scene_set_spheres": ("int", 7), "ptr_scene_set_rects": ("int", 7), "ptr_debug_dynamic_update_rows": ("int", 8)}
    assert set(found) == set(pt.DEFORM_SYMBOLS)
    lib = pt.load_library()
    for name, (kind, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is (C.c_int if kind == "int" else C.c_uint32), name
    assert not set(pt.DEFORM_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.FRAME_SYMBOLS) | set(pt.DYNAMIC_SYMBOLS))
    # the ctypes mirrors have the header's sizes and offsets, and the selectors the header's values
    names = ["PTR_DYNAMIC_DEFORMABLE", "PTR_DYNAMIC_PRIMITIVES"] + ["PTR_SCATTER_" + re.sub(r"(?<!^)(?=[A-Z])", "_", n).upper() for n in pt.SCATTER_ARRAYS]
    arrays = {"rects": "RECTS", "rectLights": "RECT_LIGHTS", "spheres": "SPHERES", "objPos": "OBJ_POS", "objNrm": "OBJ_NRM", "objTan": "OBJ_TAN"}
    tables = {"info": "INFO", "meshCorners": "MESH_CORNERS", "rectTriLeaf": "RECT_TRI_LEAF", "sphereLeaf": "SPHERE_LEAF", "tris": "TRIS",
              "triNormals": "TRI_NORMALS", "spheres": "SPHERES", "rects": "RECTS", "rectLights": "RECT_LIGHTS"}
    names += ["PTR_SCENE_ARRAY_" + v for v in arrays.values()] + ["PTR_DYNAMIC_TABLE_" + v for v in tables.values()]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_deform.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(PtrMeshVertices), sizeof(PtrSphereUpdate), sizeof(PtrRectUpdate), offsetof(PtrMeshVertices, positions), "
                   "offsetof(PtrMeshVertices, tangents), offsetof(PtrSphereUpdate, centerRadius), offsetof(PtrRectUpdate, corner), "
                   "offsetof(PtrRectUpdate, normalAndPlane));\n" + "".join('std::printf("%%d\\n", (int)%s);\n' % n for n in names) + "}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    mv, su, ru = pt.PtrMeshVertices, pt.PtrSphereUpdate, pt.PtrRectUpdate
    assert [int(s) for s in lines[0].split()] == [C.sizeof(mv), C.sizeof(su), C.sizeof(ru), mv.positions.offset, mv.tangents.offset,
                                                  su.centerRadius.offset, ru.corner.offset, ru.normalAndPlane.offset] == [32, 32, 80, 8, 24, 16, 16, 64]
    values = [int(s) for s in lines[1:1 + len(names)]]
    want = [pt.PTR_DYNAMIC_DEFORMABLE, pt.PTR_DYNAMIC_PRIMITIVES] + list(range(len(pt.SCATTER_ARRAYS))) + \
           [pt.SCENE_ARRAYS[k][0] for k in arrays] + [pt.DYNAMIC_TABLES[k][0] for k in tables]
    assert values == want
    assert pt.DYNAMIC_TABLES["info"][0] == 12 and pt.DYNAMIC_TABLES["sphereLeaf"][0] == 15, "the new tables follow INFO: the old numbers stay"


def test_null_arguments_unknown_flags_and_a_missing_device_are_refused():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    out = C.c_void_p()
    desc = pt.PtrSceneDesc()
    assert lib.ptr_scene_upload_dynamic_ex(None, 0, 3, C.byref(out), err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_upload_dynamic_ex(C.byref(desc), 0, 4, C.byref(out), err, len(err)) == 1 and b"unknown flag" in err.value
    for fn in (lib.ptr_scene_set_mesh_vertices, lib.ptr_scene_set_spheres, lib.ptr_scene_set_rects):
        assert fn(None, None, 0, None, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_dynamic_flags(None) == 0
    if pt.device_count() < 1:
        assert lib.ptr_scene_upload_dynamic_ex(C.byref(desc), 0, 3, C.byref(out), err, len(err)) == 2
        assert err.value.decode().startswith("ptr_scene_upload_dynamic_ex: no HIP device") and not out.value
    n = C.c_uint64(0)
    assert lib.ptr_debug_dynamic_update_rows(None, 0, None, None, 0, C.byref(n), err, len(err)) == 1


# --------------------------------------------------------------------------- the preparation did not change
OLD_TABLES = [k for k, v in pt.DYNAMIC_TABLES.items() if v[0] <= 12 and k != "info"]


@pytest.mark.parametrize("key", ["A", "D"])
def test_preparation_is_what_the_commit_before_produced(key, tmp_path):
    """tests/golden/vectors/dynamic_tables_parent.json: size and SHA-256 of every table ptr_debug_dynamic_tables returned for scenes A and D
    in a build of the commit before this header existed, and its info words; dynamic_tables_parent_A.npz: scene A's tables themselves
    (scene D's are 9 MB, past what the tree stores).  Equal digests of equal sizes are taken for equal bytes."""
    want = json.load(open(os.path.join(VECTORS, "dynamic_tables_parent.json")))[key]
    host = ts.scene_a() if key == "A" else ts.scene_d(tmp_path)
    got = pt.debug_dynamic_tables(host.desc, OLD_TABLES + ["info"])
    assert got["info"] == want["info"]
    assert set(OLD_TABLES) == set(want) - {"info"}
    stored = np.load(os.path.join(VECTORS, "dynamic_tables_parent_A.npz")) if key == "A" else None
    for name in OLD_TABLES:
        a = np.ascontiguousarray(got[name])
        assert a.nbytes == want[name]["bytes"], name
        assert hashlib.sha256(a.tobytes()).hexdigest() == want[name]["sha256"], name
        if stored is not None:
            assert a.dtype == stored[name].dtype and a.tobytes() == np.ascontiguousarray(stored[name]).tobytes(), name


# --------------------------------------------------------------------------- the new tables
def two_mesh_scene(tmp):
    ts._write_obj(tmp / "m0.obj", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0), (1.2, 1.1, 0.3)], [(0, 1, 2), (2, 1, 3)])
    ts._write_obj(tmp / "m1.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], [(4, 0, 1), (0, 2, 3), (3, 1, 4), (2, 4, 0)])
    p = tmp / "two.scene"
    p.write_text(ts.HEAD + "mesh path=m0.obj material=0\nmesh path=m1.obj translate=3,0,0 material=0\n")
    return ts.load(p, str(tmp))


@pytest.mark.parametrize("key", ["textured", "two", "strip"])
def test_mesh_corners_are_the_descriptions_indices(key, tmp_path):
    host = {"textured": lambda: pt.HostScene.load(os.path.join(ts.GOLDEN, "textured.scene"), ts.GOLDEN), "two": lambda: two_mesh_scene(tmp_path),
            "strip": lambda: dsc.scene_strip(tmp_path)}[key]()
    t = pt.debug_dynamic_tables(host.desc, ["meshCorners", "meshTris", "meshTriOffsets", "tris"])
    off, tris, corners = t["meshTriOffsets"], t["meshTris"], t["meshCorners"]
    assert len(corners) == len(tris) and len(off) == host.desc.meshCount + 1
    words = t["tris"].view(np.uint32)
    checked = 0
    for m in range(host.desc.meshCount):
        idx = dsc.mesh_data(host, m)[3]
        assert off[m + 1] - off[m] == len(idx)
        for e in range(off[m], off[m + 1]):
            k = tris[e]
            assert words[k, 1, 3] >> 30 == 0 and words[k, 1, 3] & 0x3FFFFFF == m, "the entry names a triangle of its mesh"
            number = words[k, 2, 3]   # the triangle's number within its mesh
            assert np.array_equal(corners[e], idx[number]), (m, e)
            checked += 1
    assert checked == len(tris) and (key != "strip" or checked == 257)


@pytest.mark.parametrize("key", ["A", "B"])
def test_rect_and_sphere_tables_invert_the_leaf_order(key):
    host = ts.scene_a() if key == "A" else ts.scene_b()
    t = pt.debug_dynamic_tables(host.desc, ["rectTriLeaf", "sphereLeaf", "tris", "spheres"])
    words = t["tris"].view(np.uint32)
    assert len(t["rectTriLeaf"]) == host.desc.rectCount and len(t["sphereLeaf"]) == host.desc.sphereCount
    for r in range(host.desc.rectCount):
        for half in range(2):
            k = t["rectTriLeaf"][r, half]
            assert words[k, 1, 3] >> 30 == 2 and words[k, 1, 3] & 0x3FFFFFF == r and words[k, 2, 3] == 2 * r + half
    assert len(np.unique(t["sphereLeaf"])) == host.desc.sphereCount
    for s in range(host.desc.sphereCount):
        assert np.array_equal(t["spheres"][t["sphereLeaf"][s]], np.array(list(host.desc.spheres[s].centerRadius), np.float32))
    assert host.desc.sphereCount > 0 and (key != "A" or host.desc.rectCount == 6)


# --------------------------------------------------------------------------- the row writers
def rows_of_fresh(desc, kind, index):
    """The rows of sphere / rectangle `index` in the host preparation of `desc`, as {(array, row offset within the primitive): bits}."""
    t = pt.debug_dynamic_tables(desc, ["tris", "triNormals", "triBounds", "spheres", "sphereBounds", "rects", "rectLights", "rectTriLeaf", "sphereLeaf"])
    out = {}
    if kind == "sphere":
        slot = t["sphereLeaf"][index]
        out[("spheres", 0)] = t["spheres"][slot]
        for q in range(2):
            out[("sphereBounds", q)] = t["sphereBounds"][slot, q]
        return out, {"spheres": slot, "sphereBounds": slot * 2}
    base = {}
    for half in range(2):
        k = int(t["rectTriLeaf"][index, half])
        for c in range(3):
            out[("tris", half, c)] = t["tris"][k, c]
            out[("triNormals", half, c)] = t["triNormals"][k, c]
        for q in range(2):
            out[("triBounds", half, q)] = t["triBounds"][k, q]
        base[half] = k
    for q in range(5):
        out[("rects", q)] = t["rects"][index, q]
    lights = t["rectLights"].view(np.uint32)
    for li in range(len(lights)):
        if lights[li, 2, 3] == index:
            for q in range(11):
                out[("rectLights", q)] = t["rectLights"][li, q]
            base["light"] = li
    return out, base


def keyed(rows, base, kind):
    """The update's rows under the keys of rows_of_fresh: `base` locates the primitive in the (unchanged) leaf order of the original."""
    out = {}
    for array, row, value in rows:
        if kind == "sphere":
            out[(array, row - base[array])] = value
        elif array in ("tris", "triNormals"):
            half = 0 if row // 3 == base[0] else 1
            assert row // 3 == base[half]
            out[(array, half, row % 3)] = value
        elif array == "triBounds":
            half = 0 if row // 2 == base[0] else 1
            assert row // 2 == base[half]
            out[(array, half, row % 2)] = value
        elif array == "rects":
            out[(array, row - 5 * base["index"])] = value
        else:
            out[(array, row - 11 * base["light"])] = value
    return out


RECT_MOVES = {
    # the light of scene A, moved and turned so that cross(edgeU, edgeV) points along the stored normal (no flip) ...
    "light, same winding": (5, dict(corner=(100.0, 300.0, 120.0), edgeU=(130.0, 10.0, 0.0), edgeV=(0.0, 20.0, 90.0), normal=(0.1, -1.0, 0.2))),
    # ... and against it (the winding flips)
    "light, flipped winding": (5, dict(corner=(100.0, 300.0, 120.0), edgeU=(0.0, 20.0, 90.0), edgeV=(130.0, 10.0, 0.0), normal=(0.1, -1.0, 0.2))),
    "wall, flipped winding": (1, dict(corner=(20.0, -30.0, 10.0), edgeU=(0.0, 500.0, 40.0), edgeV=(35.0, 0.0, 600.0), normal=(-1.0, 0.0, 0.0))),
    "wall, same winding": (4, dict(corner=(0.0, 0.0, 700.0), edgeU=(555.0, 0.0, 30.0), edgeV=(0.0, 555.0, 0.0), normal=(0.0, 0.0, 1.0))),
}


@pytest.mark.parametrize("name", list(RECT_MOVES))
def test_update_rows_of_a_rectangle_equal_the_preparations(name):
    host = ts.scene_a()
    index, move = RECT_MOVES[name]
    u = pt.rect_update(index, **move)
    n = np.cross(np.array(move["edgeU"]), np.array(move["edgeV"]))
    assert (np.dot(n, np.array(move["normal"])) < 0) == ("flipped" in name)
    _, base = rows_of_fresh(host.desc, "rect", index)   # where the primitive lives in the original's leaf order
    base["index"] = index
    got = keyed(pt.debug_dynamic_update_rows(host.desc, u), base, "rect")
    want, _ = rows_of_fresh(dsc.Changed(host, rects={index: u}).desc, "rect", index)
    assert set(got) == set(want) and (("rectLights", 0) in want) == name.startswith("light")
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k, got[k], want[k])
    original, _ = rows_of_fresh(host.desc, "rect", index)
    assert any(not np.array_equal(original[k], want[k]) for k in want)


@pytest.mark.parametrize("row", [(120.0, 300.0, 90.0, -35.5), (1.0e4, -2.0e3, 17.0, 3.25)], ids=["negative radius", "far away"])
def test_update_rows_of_a_sphere_equal_the_preparations(row):
    host = ts.scene_a()
    u = pt.PtrSphereUpdate()
    u.sphereIndex = 0
    u.centerRadius[:] = list(row)
    _, base = rows_of_fresh(host.desc, "sphere", 0)
    got = keyed(pt.debug_dynamic_update_rows(host.desc, u), base, "sphere")
    want, _ = rows_of_fresh(dsc.Changed(host, spheres={0: row}).desc, "sphere", 0)
    assert set(got) == set(want) and len(want) == 3
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, got[k], want[k])
    if row[3] < 0:
        assert want[("sphereBounds", 0)][0] < row[0] < want[("sphereBounds", 1)][0], "the bounds take |radius|"


def test_what_the_host_half_refuses():
    host = ts.scene_a()
    good = dict(corner=(1.0, 2.0, 3.0), edgeU=(1.0, 0.0, 0.0), edgeV=(0.0, 1.0, 0.0), normal=(0.0, 0.0, 1.0))
    cases = []
    u = pt.rect_update(host.desc.rectCount, **good)
    cases.append((u, "out of range"))
    u = pt.rect_update(0, **good)
    u.corner[1] = float("nan")
    cases.append((u, "non-finite"))
    u = pt.rect_update(0, **dict(good, edgeV=(2.0, 0.0, 0.0)))
    cases.append((u, r"cross\(edgeU, edgeV\) of length zero"))
    u = pt.rect_update(0, **good)
    u.normalAndPlane[:] = [0.0, 0.0, 0.0, 0.0]
    cases.append((u, "normal of length zero"))
    s = pt.PtrSphereUpdate()
    s.sphereIndex = 1
    cases.append((s, "out of range"))
    s = pt.PtrSphereUpdate()
    s.centerRadius[:] = [0.0, float("inf"), 0.0, 1.0]
    cases.append((s, "non-finite"))
    for update, pattern in cases:
        with pytest.raises(pt.PtrError, match=pattern):
            pt.debug_dynamic_update_rows(host.desc, update)
