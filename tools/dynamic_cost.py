#!/usr/bin/env python3
"""What moving a mesh of a dynamic scene (include/ptr_dynamic.h) costs, in one job on one GPU.

  update   ptr_scene_set_mesh_transforms on BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3] (scenes/knot_glass.scene):
           the call's wall time and its four kernel groups by device events (bake, refit, quantise, wide), median of 5 after 2 warm-ups,
           against ptr_scene_upload of the same moved description.  Per group the least bytes it moves, over its time, against the HBM
           peak: the bake reads two 48 B corner records and a list word and writes 48 + 48 + 32 B per triangle; the refit reads and
           writes each 64 B node, and reads 32 B per leaf primitive and 64 B per internal child; the quantiser reads 64 B and writes 32 B
           per node; the wide copy reads a source word and a 16 B record and rewrites a 16 B place.
  quality  the configs[1] mesh turned by 5, 45 and 180 degrees about the vertical axis through its centre: k_extend + k_connect kernel
           time per frame (1920x1080, depth 8, 16 spp) on the refitted scene over a fresh upload at the same pose.  The ratio says when
           re-uploading pays.
  memory   what a dynamic scene keeps beside a static one, in bytes per triangle and per node, from the array sizes.

  python tools/dynamic_cost.py [--out profiles/dynamic_cost.json]

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cov_cost import HBM_PEAK_BYTES_PER_S  # noqa: E402

EMPTY, LEAF = 0xFFFFFFFF, 0x80000000


class Moved:
    """The description of `host` with other localToWorld matrices ({mesh: 4x4, row / column})."""

    def __init__(self, pt, host, matrices):
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


def matrix_of(host, mesh=0):
    return np.array(list(host.desc.meshes[mesh].localToWorld), np.float32).reshape(4, 4).T.astype(np.float64)


def turned(host, degrees, mesh=0):
    """The mesh's matrix turned about the vertical axis through the mesh's world-space centre."""
    base = matrix_of(host, mesh)
    d = host.desc.meshes[mesh]
    pos = np.ctypeslib.as_array(d.positions, (d.vertexCount, 3)).astype(np.float64)
    centre = (base[:3, :3] @ ((pos.min(axis=0) + pos.max(axis=0)) / 2)) + base[:3, 3]
    a = np.radians(degrees)
    r = np.eye(4)
    r[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    to, back = np.eye(4), np.eye(4)
    to[:3, 3], back[:3, 3] = -centre, centre
    return (back @ r @ to @ base).astype(np.float32)


def update_cost(pt, scene_path, rounds, warmups):
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(scene_path, scenes)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    tables = pt.debug_dynamic_tables(host.desc, ["info", "nodes", "wideSource", "meshTriOffsets"])
    refs = tables["nodes"].reshape(-1, 16).view(np.uint32)[:, [3, 7]]
    leaf = (refs != EMPTY) & ((refs & LEAF) != 0)
    internal = (refs != EMPTY) & ((refs & LEAF) == 0)
    leaf_prims = int((((refs[leaf] >> 26) & 0xF) + 1).sum())
    nodes, tris = tables["info"]["nodes"], int(tables["meshTriOffsets"][1] - tables["meshTriOffsets"][0])
    used = int((tables["wideSource"] != EMPTY).sum())
    group_bytes = {"bake": tris * (48 + 48 + 4 + 48 + 48 + 32), "refit": nodes * (64 + 64 + 4) + leaf_prims * 32 + int(internal.sum()) * 64,
                   "quantise": nodes * (64 + 32) if tables["info"]["quantized"] else 0, "wide": tables["wideSource"].size * 4 + used * 48}
    poses = [turned(host, 10.0 * (k + 1)) for k in range(rounds + warmups)]
    infos, walls = [], []
    for k, pose in enumerate(poses):
        t0 = time.perf_counter()
        info = dev.set_mesh_transforms({0: pose})
        if k >= warmups:
            walls.append((time.perf_counter() - t0) * 1e3)
            infos.append(info)
    uploads = []
    for k in range(min(rounds, 3)):
        moved = Moved(pt, host, {0: poses[-1]})
        t0 = time.perf_counter()
        fresh = pt.DeviceScene(moved.desc, 0, keepalive=moved)
        uploads.append((time.perf_counter() - t0) * 1e3)
        fresh.close()
    med = lambda xs: round(statistics.median(xs), 4)
    groups = {}
    for name, key in (("bake", "bakeMs"), ("refit", "refitMs"), ("quantise", "quantiseMs"), ("wide", "wideMs")):
        ms = med([i[key] for i in infos])
        groups[name] = {"ms": ms, "min_bytes": group_bytes[name],
                        "fraction_of_hbm_peak": round(group_bytes[name] / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 5) if ms > 0 else None}
    a = dev.arrays()
    static_bytes = sum(a[k].nbytes for k in ("tris", "triNormals", "triUv", "triTangent", "qnodes", "wnodes"))
    extra_tri = 48 + 48 + 32 + 4   # object-space positions and normals, padded bounds, list word
    extra_node = (64 if tables["info"]["quantized"] else 0) + 4 + (tables["wideSource"].size * 4 / max(nodes, 1))
    report = {"scene": os.path.relpath(scene_path, ROOT), "mesh_triangles": tris, "nodes": nodes, "levels": tables["info"]["levels"],
              "wide_nodes": tables["info"]["wide_nodes"], "set_mesh_transforms_ms": med(walls), "set_mesh_transforms_ms_all": [round(w, 4) for w in walls],
              "call_seconds_reported": med([i["totalSeconds"] for i in infos]), "groups": groups,
              "upload_of_moved_description_ms": med(uploads), "upload_over_update": round(med(uploads) / med(walls), 1),
              "cell_over_extent": infos[-1]["cellOverExtent"],
              "memory": {"static_geometry_bytes": int(static_bytes), "extra_bytes_per_triangle": extra_tri, "extra_bytes_per_node": round(extra_node, 2),
                         "extra_bytes": int(a["triBounds"].nbytes + a["sphereBounds"].nbytes + 2 * a["tris"].nbytes + tris * 4 + nodes * 4
                                            + tables["wideSource"].size * 4 + (a["boxes"].nbytes if tables["info"]["quantized"] else 0))}}
    dev.close()
    return report


def refit_quality(pt, width, height, spp):
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=width, height=height, max_depth=8, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    out = []
    for degrees in (5.0, 45.0, 180.0):
        pose = turned(host, degrees)
        dev.set_mesh_transforms({0: pose})
        moved = Moved(pt, host, {0: pose})
        fresh = pt.DeviceScene(moved.desc, 0, keepalive=moved)
        ms = {"refitted": [], "fresh": []}
        for k in range(4):   # alternating; the first pair warms up
            for name, scene in (("refitted", dev), ("fresh", fresh)):
                st = scene.render(s, spp)[1]
                if k:
                    ms[name].append(st.traceKernelMs + st.shadowKernelMs)
        fresh.close()
        r, f = statistics.median(ms["refitted"]), statistics.median(ms["fresh"])
        out.append({"degrees": degrees, "extend_connect_ms_refitted": round(r, 3), "extend_connect_ms_fresh": round(f, 3), "refitted_over_fresh": round(r / f, 4)})
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_cost.json"), help="the report file")
    args = ap.parse_args()
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    from scenes.gen_assets import ensure_assets, ensure_large_asset

    ensure_assets()
    scenes = os.path.join(ROOT, "scenes")
    updates = []
    for name in ("cornell_mesh.scene", "knot_glass.scene"):
        path = os.path.join(scenes, name)
        with open(path) as f:
            for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
                ensure_large_asset(asset)
        updates.append(update_cost(pt, path, args.rounds, args.warmups))
    report = {"timing": "wall time of the call and device events around its kernel groups; median of %d after %d warm-ups" % (args.rounds, args.warmups),
              "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "update": updates,
              "refit_quality": {"scene": "scenes/cornell_mesh.scene", "resolution": [args.width, args.height], "max_depth": 8, "spp": args.spp,
                                "timing": "k_extend + k_connect kernel ms per frame (PtrRenderStats), median of 3 alternating frames after a warm-up",
                                "poses": refit_quality(pt, args.width, args.height, args.spp)},
              "not_measured": "BASELINE configs[4] (29 M triangles): its generated mesh was not at hand in this job"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
