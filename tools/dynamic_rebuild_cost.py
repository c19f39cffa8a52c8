#!/usr/bin/env python3
"""What rebuilding the tree above the leaves of a dynamic scene (include/ptr_rebuild.h) costs and what it buys, in one job on one GPU.

  call     ptr_scene_rebuild_tree on BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3] (scenes/knot_glass.scene), mesh 0
           turned by 45 degrees: the call's wall time and its kernel groups by device events (keys + sort, topology + numbering,
           heights + fit, quantise, wide), median of 5 after 2 warm-ups (the first call also allocates the second set of arrays:
           reported apart), against ptr_scene_tree_cost alone and an upload of the same description.
  quality  per config, three trees at the same pose - the refitted one, the rebuilt one (installed whatever its cost) and a fresh
           upload's - at 5 and 45 degrees about the vertical axis and under one strong deformation, a twist of a full turn along the
           mesh's longest axis through set_mesh_vertices_device: k_extend + k_connect kernel time per frame (1920x1080, depth 8,
           16 spp, median of 3 alternating frames after a warm-up) and tree_cost() of each.  `sah_ranks_as_time` says whether the SAH
           figure orders the refitted and the rebuilt tree as the traversal time does: PTR_REBUILD_KEEP_IF_BETTER rests on that.

  python tools/dynamic_rebuild_cost.py [--out profiles/dynamic_rebuild_cost.json]

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dynamic_cost import turned  # noqa: E402


def med(xs):
    return round(statistics.median(xs), 4)


def twisted(pos, nrm, tan, turns=1.0):
    """The mesh twisted about its longest object-space axis: a rotation that grows from 0 to `turns` full turns along it."""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u, v = (axis + 1) % 3, (axis + 2) % 3
    centre = (lo + hi) / 2
    a = 2.0 * np.pi * turns * (pos[:, axis] - lo[axis]) / max(float(hi[axis] - lo[axis]), 1e-30)
    c, s = np.cos(a), np.sin(a)

    def turn(x, about):
        out = x.astype(np.float64).copy()
        p, q = out[:, u] - about[u], out[:, v] - about[v]
        out[:, u], out[:, v] = c * p - s * q + about[u], s * p + c * q + about[v]
        return out.astype(np.float32)

    zero = np.zeros(3)
    out = [turn(pos, centre), turn(nrm, zero)]
    if tan is not None:
        t = tan.copy()
        t[:, :3] = turn(tan[:, :3], zero)
        out.append(t)
    return tuple(out)


def call_cost(pt, host, rounds, warmups):
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    walls, infos, costs = [], [], []
    first = None
    for k in range(rounds + warmups):
        dev.set_mesh_transforms({0: turned(host, 45.0 + k)})
        t0 = time.perf_counter()
        dev.tree_cost()
        t1 = time.perf_counter()
        info = dev.rebuild_tree(keep_if_better=False)
        t2 = time.perf_counter()
        if k == 0:
            first = round((t2 - t1) * 1e3, 4)
        if k >= warmups:
            costs.append((t1 - t0) * 1e3)
            walls.append((t2 - t1) * 1e3)
            infos.append(info)
    uploads = []
    for _ in range(3):
        t0 = time.perf_counter()
        fresh = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
        uploads.append((time.perf_counter() - t0) * 1e3)
        fresh.close()
    dev.close()
    groups = {name: med([i[key] for i in infos]) for name, key in (("keys_sort", "keysSortMs"), ("topology_numbering", "topologyMs"), ("heights_fit", "fitMs"),
                                                                    ("quantise", "quantiseMs"), ("wide", "wideMs"))}
    last = infos[-1]
    return {"rebuild_tree_ms": med(walls), "rebuild_tree_ms_all": [round(w, 4) for w in walls], "first_call_ms": first, "groups_ms": groups,
            "outside_the_kernel_groups_ms": round(med(walls) - sum(groups.values()), 4), "tree_cost_ms": med(costs), "upload_dynamic_ms": med(uploads),
            "leaves": last["leaves"], "nodes": last["nodes"], "levels": last["levels"], "wide_nodes": last["wideNodes"], "wide_depth": last["wideDepth"]}


def three_trees(pt, dsc, host, s, spp, name, refitted, fresh_holder):
    """`refitted`: a dynamic scene already at the pose; its twin is rebuilt; `fresh_holder`: the description at the same pose."""
    fresh = pt.DeviceScene(fresh_holder.desc, 0, keepalive=fresh_holder, dynamic=True, deformable=True)
    scenes ={"refitted": refitted[0], "rebuilt": refitted[1], "fresh": fresh}
    info = refitted[1].rebuild_tree(keep_if_better=False)
    ms = {k: [] for k in scenes}
    order = list(scenes)
    for k in range(4):   # alternating, each round starting with another tree; the first round warms up
        for key in order[k % 3:] + order[:k % 3]:
            st = scenes[key].render(s, spp)[1]
            if k:
                ms[key].append(st.traceKernelMs + st.shadowKernelMs)
    out = {"case": name, "extend_connect_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()},
           "tree_cost": {k: round(scene.tree_cost(), 4) for k, scene in scenes.items()},
           "levels": {"rebuilt": info["levels"]}, "rebuild_ms": round(info["totalSeconds"] * 1e3, 4)}
    t, c = out["extend_connect_ms"], out["tree_cost"]
    out["rebuilt_over_refitted_ms"] = round(t["rebuilt"] / t["refitted"], 4)
    out["refitted_over_fresh_ms"] = round(t["refitted"] / t["fresh"], 4)
    out["rebuilt_over_fresh_ms"] = round(t["rebuilt"] / t["fresh"], 4)
    out["keep_if_better_would_install"] = bool(c["rebuilt"] < c["refitted"])
    out["sah_ranks_as_time"] = bool((c["rebuilt"] < c["refitted"]) == (t["rebuilt"] < t["refitted"]))
    out["sah_ranks_all_three_as_time"] = bool(sorted(t, key=t.get) == sorted(c, key=c.get))
    fresh.close()
    return out


def quality(pt, torch, dsc, host, width, height, spp):
    s = host.settings_for(width=width, height=height, max_depth=8, seed=1337)
    make = lambda: pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True, deformable=True)
    out = []
    for degrees in (5.0, 45.0):
        pair = (make(), make())
        pose = turned(host, degrees)
        for d in pair:
            d.set_mesh_transforms({0: pose})
        out.append(three_trees(pt, dsc, host, s, spp, "turned %g degrees" % degrees, pair, dsc.Changed(host, matrices={0: pose})))
        for d in pair:
            d.close()
    pos, nrm, tan, _ = dsc.mesh_data(host, 0)
    data = twisted(pos, nrm, tan)
    tensors = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in data)
    torch.cuda.synchronize()
    pair = (make(), make())
    for d in pair:
        d.set_mesh_vertices_device({0: tensors})
    out.append(three_trees(pt, dsc, host, s, spp, "twisted one full turn along the longest axis (set_mesh_vertices_device)", pair,
                           dsc.Changed(host, vertices={0: data})))
    for d in pair:
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_rebuild_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import deform_scenes as dsc
    from scenes.gen_assets import ensure_assets, ensure_large_asset

    if pt.device_count() < 1:
        raise SystemExit("tools/dynamic_rebuild_cost.py needs a GPU")
    ensure_assets()
    scenes = os.path.join(ROOT, "scenes")
    reports = []
    for name in ("cornell_mesh.scene", "knot_glass.scene"):
        path = os.path.join(scenes, name)
        with open(path) as f:
            for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
                ensure_large_asset(asset)
        host = pt.HostScene.load(path, scenes)
        reports.append({"scene": os.path.relpath(path, ROOT), "call": call_cost(pt, host, args.rounds, args.warmups),
                        "quality": quality(pt, torch, dsc, host, args.width, args.height, args.spp)})
    report = {"timing": "wall time of the call and device events around its kernel groups, median of %d after %d warm-ups; quality: k_extend + k_connect "
                        "kernel ms per frame (PtrRenderStats), %dx%d, depth 8, %d spp, median of 3 alternating frames after a warm-up"
                        % (args.rounds, args.warmups, args.width, args.height, args.spp),
              "scenes": reports}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
