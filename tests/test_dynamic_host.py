"""CPU tests of dynamic scenes (include/ptr_dynamic.h): the exported surface, the refit schedule, and the claim the device tests rest on -
that a refit of the builder's own tree from the leaf-order padded bounds (tests/dynamic_ref.py), the shared quantiser and the wide-source
copy reproduce the builder's float, quantised and four-wide nodes bit for bit.  No GPU."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_ref as dr
import traversal_scenes as ts

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_dynamic_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "ptr_dynamic.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: 0 if args.strip() in ("", "void") else args.count(",") + 1
             for name, args in re.findall(r"\bint\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {"ptr_scene_upload_dynamic": 5, "ptr_scene_set_mesh_transforms": 7, "ptr_scene_is_dynamic": 1,
                     "ptr_debug_scene_arrays": 5, "ptr_debug_dynamic_tables": 7}
    assert set(found) == set(pt.DYNAMIC_SYMBOLS)
    lib = pt.load_library()
    for name, count in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is C.c_int, name
    assert not set(pt.DYNAMIC_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.FRAME_SYMBOLS))
    # the ctypes mirrors have the header's sizes: a one-line sizeof program
    assert C.sizeof(pt.PtrMeshTransform) == 72
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "ptr_dynamic.h"\nint main() { std::printf("%zu %zu\\n", sizeof(PtrMeshTransform), sizeof(PtrUpdateInfo)); }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(s) for s in sizes] == [C.sizeof(pt.PtrMeshTransform), C.sizeof(pt.PtrUpdateInfo)] == [72, 128]
    assert pt.PtrUpdateInfo.trianglesMoved.offset == 40 and pt.PtrUpdateInfo.sceneLo.offset == 72 and pt.PtrUpdateInfo.cellOverExtent.offset == 120


def test_null_arguments_and_a_missing_device_are_refused():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    out = C.c_void_p()
    desc = pt.PtrSceneDesc()
    assert lib.ptr_scene_upload_dynamic(None, 0, C.byref(out), err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_upload_dynamic(C.byref(desc), 0, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_set_mesh_transforms(None, None, 0, None, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_scene_is_dynamic(None) == 0
    if pt.device_count() < 1:
        assert lib.ptr_scene_upload_dynamic(C.byref(desc), 0, C.byref(out), err, len(err)) == 2
        assert err.value.decode().startswith("ptr_scene_upload_dynamic: no HIP device") and not out.value
    size = C.c_uint64(0)
    assert lib.ptr_debug_scene_arrays(None, 0, None, 0, C.byref(size)) == 1
    assert lib.ptr_debug_dynamic_tables(None, 0, None, 0, C.byref(size), err, len(err)) == 1
    assert lib.ptr_debug_dynamic_tables(C.byref(desc), 99, None, 0, C.byref(size), err, len(err)) == 1 and b"no such table" in err.value


# --------------------------------------------------------------------------- the tables
SCENES = ["A", "B", "D", "E", "F-triangle", "F-sphere", "F-coincident", "F-flat", "F-empty"]
FORMATS = {"default": {}, "PTR_WIDE_NODES=0": {"PTR_WIDE_NODES": "0"}, "PTR_WIDE_NODES=2": {"PTR_WIDE_NODES": "2"}}


def _host(key, tmp):
    if key == "A":
        return ts.scene_a()
    if key == "B":
        return ts.scene_b()
    if key == "D":
        return ts.scene_d(tmp)
    if key == "E":
        return ts.scene_e(tmp, count=20000)
    return ts.scene_f(tmp, key[2:])


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cache = {}

    def get(key, fmt="default"):
        if (key, fmt) not in cache:
            host = _host(key, tmp_path_factory.mktemp("dyn_" + key.replace("-", "_")))
            old = {k: os.environ.get(k) for k in FORMATS[fmt]}
            os.environ.update(FORMATS[fmt])
            try:
                cache[(key, fmt)] = (host, pt.debug_dynamic_tables(host.desc))
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return cache[(key, fmt)]
    return get


@pytest.mark.parametrize("key", SCENES)
def test_schedule_orders_children_before_parents(tables, key):
    _, t = tables(key)
    info, sched, off = t["info"], t["schedule"], t["levelOffsets"]
    n = info["nodes"]
    assert len(off) == info["levels"] + 1 and off[0] == 0 and off[-1] == n == len(sched) and (np.diff(off.astype(np.int64)) > 0).all()
    assert np.array_equal(np.sort(sched), np.arange(n, dtype=np.uint32)), "every node is in exactly one level"
    if key == "F-empty":
        assert n == 0 and info["levels"] == 0
        return
    level_of = np.zeros(n, np.int64)
    for l in range(info["levels"]):
        level_of[sched[off[l]:off[l + 1]]] = l
    assert np.array_equal(level_of, dr.heights(t["nodes"]))
    refs = dr.refs_of(t["nodes"])
    internal = (refs != dr.EMPTY) & ((refs & dr.LEAF) == 0)
    for c in range(2):
        kids = refs[internal[:, c], c]
        assert (level_of[kids] < level_of[internal[:, c]]).all(), "internal children are in levels below their parent"
    assert not internal[level_of == 0].any(), "level 0 has only leaf children"
    assert 1 <= info["levels"] <= info["max_depth"]


@pytest.mark.parametrize("key", SCENES)
def test_refit_quantiser_and_wide_copy_reproduce_the_builder(tables, key):
    """What licenses bit equality on the device: the tables alone give back the builder's arrays."""
    _, t = tables(key)
    # boxes scrambled first, so that the refit has to produce every one of them
    start = t["nodes"].reshape(-1, 16).copy()
    start[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]] = np.float32(123.25)
    empty = dr.refs_of(t["nodes"]) == dr.EMPTY
    for c in range(2):   # (an empty child keeps its record)
        cols = [c * 8, c * 8 + 1, c * 8 + 2, c * 8 + 4, c * 8 + 5, c * 8 + 6]
        start[np.ix_(empty[:, c], cols)] = t["nodes"].reshape(-1, 16)[np.ix_(empty[:, c], cols)]
    refit = dr.refit(start, t["schedule"], t["levelOffsets"], t["triBounds"], t["sphereBounds"])
    assert np.array_equal(refit.view(np.uint32), t["nodes"].view(np.uint32)), "refit of the padded bounds != the builder's float nodes"
    if t["info"]["nodes"]:
        lo, hi = dr.root_box(t["nodes"])
        assert np.array_equal(dr.grid_of(lo, hi).view(np.uint32), t["grid"].view(np.uint32)), "grid rule on the root box != the builder's grid"
    assert np.array_equal(t["requantised"], t["qnodes"]), "shared quantiser != the builder's qnodes"
    assert np.array_equal(dr.quantise(t["nodes"], t["grid"]), t["qnodes"]), "float64 restatement of the quantiser != the builder's qnodes"
    for fmt in FORMATS:
        _, tf = tables(key, fmt)
        assert np.array_equal(tf["qnodes"], t["qnodes"])
        if fmt == "PTR_WIDE_NODES=0" or not tf["info"]["quantized"]:
            assert tf["info"]["wide_nodes"] == 0 and len(tf["wnodes"]) == 0 and len(tf["wideSource"]) == 0
            continue
        assert tf["info"]["wide_nodes"] == len(tf["wnodes"]) == len(tf["wideSource"]) > 0
        blank = tf["wnodes"].copy()
        used = tf["wideSource"] != dr.NO_SOURCE
        blank[used, :3] = 0xDEADBEEF
        assert np.array_equal(dr.wide_copy(blank, tf["qnodes"], tf["wideSource"]), tf["wnodes"]), fmt
        # unused places are the inverted box with an empty reference
        assert np.array_equal(tf["wnodes"][~used], np.broadcast_to(np.array([0xFFFFFFFF, 0x0000FFFF, 0, 0xFFFFFFFF], np.uint32), (int((~used).sum()), 4)))


@pytest.mark.parametrize("key", ["A", "D", "E"])
def test_mesh_lists_name_every_mesh_triangle_once(tables, key):
    host, t = tables(key)
    off, tris = t["meshTriOffsets"], t["meshTris"]
    assert len(off) == host.desc.meshCount + 1 and off[-1] == len(tris)
    assert len(np.unique(tris)) == len(tris) and (tris < t["info"]["triangles"]).all()
    assert len(tris) == t["info"]["triangles"] - 2 * host.desc.rectCount


# --------------------------------------------------------------------------- the builder did not change
def test_builder_output_is_what_it_was():
    """Factoring the grid rule and the quantiser out of BuildFlatBvh changed nothing: the figures of scenes A and D as the commit before
    dynamic scenes printed them."""
    want = {"A": dict(nodes=624, leaves=625, sah_cost_milli=19124, wide_nodes=303, wide_depth=7, oversize=0, max_depth=13),
            "D": dict(nodes=38333, leaves=38335, sah_cost_milli=2389, wide_nodes=18822, wide_depth=11, oversize=2, max_depth=22)}
    import tempfile
    import pathlib
    with tempfile.TemporaryDirectory() as tmp:
        for key, host in (("A", ts.scene_a()), ("D", ts.scene_d(pathlib.Path(tmp)))):
            g = pt.debug_scene_geometry(host.desc)
            assert {k: g[k] for k in want[key]} == want[key], key
            assert g["box_violations"] == g["quant_violations"] == g["bad_refs"] == g["wide_problems"] == 0 and g["quantized_usable"] == 1
