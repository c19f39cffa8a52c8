"""The rebuild above the leaves without a device (include/ptr_rebuild.h): the numpy reference tree (rebuild_ref.py) is a tree the builder's
own functions accept, and the host-only probe ptr_debug_rebuild_tables - those functions on a given node array - agrees with dynamic_ref
on it and with ptr_debug_dynamic_tables on the upload's own tree.  Every comparison of arrays is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deform_scenes as dsc
import dynamic_ref as dr
import rebuild_ref as rr
import rebuild_scenes as rs

pt = rs.pt
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert "ptr_scene_rebuild_tree" in pt.REBUILD_SYMBOLS   # the restatement is of this surface: no surface, no module


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            host = rs.host_scene(key, tmp_path_factory.mktemp("rb_" + key.replace("-", "_")))
            t = pt.debug_dynamic_tables(host.desc, ["nodes", "triBounds", "sphereBounds", "schedule", "levelOffsets", "wnodes", "wideSource", "qnodes",
                                                    "grid", "info", "meshTris", "meshCorners"])
            cache[key] = (host, t, rs.reference_tree(t["nodes"], t["triBounds"], t["sphereBounds"]))
        return cache[key]
    return get


def test_the_bindings_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "ptr_rebuild.h")).read()
    found = re.findall(r"^(?:int|uint32_t) (ptr_\w+)\(", text, re.M)
    assert set(found) == set(pt.REBUILD_SYMBOLS) and len(found) == 4
    lib = pt.load_library()
    assert all(hasattr(lib, s) for s in found)
    fields = re.search(r"typedef struct PtrRebuildInfo \{(.*?)\} PtrRebuildInfo;", text, re.S).group(1)
    names = [n for decl in re.findall(r"(?:double|uint64_t|uint32_t) ([^;]+);", fields) for n in re.split(r",\s*", decl)]
    assert names == [n for n, _ in pt.PtrRebuildInfo._fields_] and C.sizeof(pt.PtrRebuildInfo) == 8 * 8 + 5 * 8 + 8
    assert pt.PTR_REBUILD_KEEP_IF_BETTER == int(re.search(r"PTR_REBUILD_KEEP_IF_BETTER = (\d+)", text).group(1))
    for table, prefix in ((pt.REBUILD_TABLES, "PTR_REBUILD_TABLE_"), (pt.REBUILD_ARRAYS, "PTR_REBUILD_ARRAY_")):
        values = sorted(int(v) for v in re.findall(prefix + r"\w+ = (\d+)", text))
        assert values == sorted(w for w, _, _ in table.values())


@pytest.mark.parametrize("key", rs.KEYS)
def test_the_reference_tree_is_a_preorder_tree_over_every_leaf(cases, key):
    _, t, (nodes, schedule, offsets) = cases(key)
    leaves = rr.leaf_table(t["nodes"])
    assert np.array_equal(leaves, pt.debug_rebuild_tables(t["nodes"], ["leafTable"])["leafTable"])
    assert np.array_equal(np.sort(leaves & rr.KEY_MASK), leaves & rr.KEY_MASK) and len(np.unique(leaves & rr.KEY_MASK)) == len(leaves)
    refs = dr.refs_of(nodes)
    if len(leaves) < 2:
        assert len(refs) == 0
        return
    assert len(refs) == len(leaves) - 1 == t["info"]["nodes"]
    assert not (refs == dr.EMPTY).any()
    is_leaf = (refs & dr.LEAF) != 0
    assert np.array_equal(np.sort(refs[is_leaf]), np.sort(leaves))   # every leaf exactly once, its word unchanged
    # preorder: node 0 is the root, the left subtree follows its parent, the right one follows the left
    size = np.ones(len(refs), np.int64)
    for i in range(len(refs) - 1, -1, -1):
        for r in refs[i]:
            if not r & dr.LEAF:
                assert r > i
                size[i] += size[int(r)]
    assert size[0] == len(refs)
    for i in range(len(refs)):
        at = i + 1
        for r in refs[i]:
            if not r & dr.LEAF:
                assert r == at
                at += size[int(r)]


@pytest.mark.parametrize("key", rs.KEYS)
def test_the_probe_on_the_reference_tree(cases, key):
    _, t, (nodes, schedule, offsets) = cases(key)
    got = pt.debug_rebuild_tables(nodes)
    assert np.array_equal(got["schedule"], schedule) and np.array_equal(got["levelOffsets"], offsets if len(nodes) else [0])
    if len(nodes) == 0:
        return
    grid = dr.grid_of(*dr.root_box(nodes))
    assert np.array_equal(got["grid"].view(np.uint32), grid.view(np.uint32))
    assert np.array_equal(grid.view(np.uint32), dr.grid_of(*dr.root_box(t["nodes"])).view(np.uint32))   # a rebuild keeps the root box
    q = dr.quantise(nodes, grid)
    assert np.array_equal(got["qnodes"], q)
    assert len(got["wnodes"]) and np.array_equal(got["wnodes"], dr.wide_copy(got["wnodes"], q, got["wideSource"]))
    assert got["wideDepth"] >= 1 and np.isclose(got["sah"], rr.tree_cost(nodes), rtol=1e-9, atol=0)


@pytest.mark.parametrize("key", rs.KEYS)
def test_the_probe_on_the_uploads_own_tree(cases, key):
    host, t, _ = cases(key)
    got = pt.debug_rebuild_tables(t["nodes"])
    assert np.array_equal(got["schedule"], t["schedule"]) and np.array_equal(got["levelOffsets"], t["levelOffsets"])
    if t["info"]["wide_nodes"]:
        assert np.array_equal(got["wnodes"], t["wnodes"]) and np.array_equal(got["wideSource"], t["wideSource"])
        assert got["wideDepth"] == t["info"]["wide_depth"]
    if t["info"]["quantized"]:
        assert np.array_equal(got["qnodes"], t["qnodes"])
    # the builder's figure: float32 areas summed in its own order; ours is float64 throughout
    want = pt.debug_scene_geometry(host.desc)["sah_cost_milli"]
    print("scene %s: probe %.9f, builder x1000 %d" % (key, got["sah"], want))
    assert int(got["sah"] * 1000.0) == want


def test_the_scrambled_quads_are_a_fair_case(cases):
    host, t, _ = cases("quads")
    pos, _ = rs.scrambled(host)
    bounds = t["triBounds"].copy()
    bounds[t["meshTris"]] = rs.padded_bounds(pos[t["meshCorners"]])   # identity localToWorld: the bake leaves the positions as they are
    assert not np.array_equal(bounds, t["triBounds"])
    refitted = dr.refit(t["nodes"], t["schedule"], t["levelOffsets"], bounds, t["sphereBounds"])
    rebuilt, _, _ = rs.reference_tree(refitted, bounds, t["sphereBounds"])
    before, after, fresh = rr.tree_cost(refitted), rr.tree_cost(rebuilt), rr.tree_cost(t["nodes"])
    print("quads: fresh %.3f, scrambled and refitted %.3f, rebuilt %.3f" % (fresh, before, after))
    assert after < before and before > 2.0 * fresh


def chain(levels):
    """A preorder tree of `levels` levels: every node a leaf on the left and the next node on the right; the last one two leaves."""
    n = np.zeros((levels, 16), np.uint32)
    for i in range(levels):
        n[i, 3] = dr.LEAF | (2 * i)
        n[i, 7] = i + 1 if i + 1 < levels else dr.LEAF | (2 * i + 1)
    f = n.view(np.float32)
    f[:, 4:7] = f[:, 12:15] = 1.0
    return f


def test_the_depth_decision():
    assert pt.debug_rebuild_tables(chain(47), ["depthCheck"])["depthCheck"] == 47   # kMaxTreeDepth - 1: the deepest tree the stacks hold
    for levels in (48, 49, 60):
        with pytest.raises(pt.PtrError, match="levels"):
            pt.debug_rebuild_tables(chain(levels), ["depthCheck"])


def test_what_the_probe_refuses():
    bad = chain(4)
    bad.view(np.uint32)[2, 7] = 1   # a reference to an earlier node
    with pytest.raises(pt.PtrError, match="no later node"):
        pt.debug_rebuild_tables(bad, ["schedule"])
    bad.view(np.uint32)[2, 7] = 9   # past the array
    with pytest.raises(pt.PtrError, match="no later node"):
        pt.debug_rebuild_tables(bad, ["sah"])
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    assert lib.ptr_debug_rebuild_tables(None, 3, 0, None, 0, None, err, len(err)) == 1 and b"null" in err.value
    size = C.c_uint64(0)
    assert lib.ptr_debug_rebuild_tables(None, 0, 99, None, 0, C.byref(size), err, len(err)) == 1 and b"no such table" in err.value
    assert lib.ptr_scene_rebuild_tree(None, 0, None, None, err, len(err)) == 1 and b"null" in err.value
    cost = C.c_double(0)
    assert lib.ptr_scene_tree_cost(None, None, C.byref(cost), err, len(err)) == 1 and b"null" in err.value
    empty = pt.debug_rebuild_tables(np.zeros((0, 16), np.float32))
    assert empty["sah"] == 0.0 and len(empty["schedule"]) == 0 and list(empty["levelOffsets"]) == [0] and len(empty["wnodes"]) == 0
