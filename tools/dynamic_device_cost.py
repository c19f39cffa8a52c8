#!/usr/bin/env python3
"""What deforming a mesh from device-resident vertex data (include/ptr_deform_device.h) costs beside the host-pointer call, in one process
on one GPU.

On the mesh of BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3] (scenes/knot_glass.scene), a sinusoidal displacement along
the normals with the phase advanced per call, three calls side by side on one scene uploaded with PTR_DYNAMIC_VERTEX_NORMALS:

  host       ptr_scene_set_mesh_vertices from numpy arrays: the path of the commit before, the baseline;
  given      ptr_scene_set_mesh_vertices_device from torch tensors, positions and normals;
  computed   ptr_scene_set_mesh_vertices_device from positions alone, the normals computed on the device.

The three take turns within a round (the same displacement each), median of 5 rounds after 2 warm-ups.  Wall time around the call, and the
call's kernel groups by device events.  PtrUpdateInfo has one figure, bakeMs, from the first kernel of a call to the end of its bake, so
the groups inside it are differences of medians: gather + bake is the host call's bakeMs (it runs nothing else there); the finiteness
kernel with the read-back of its flag words and the synchronisation is given minus host; the normals kernel is computed minus given
(the finiteness kernel reads the same number of bytes in both).  The tensors are on the device before the clock starts: that is the case
the call is for.

  python tools/dynamic_device_cost.py [--out profiles/dynamic_device_cost.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUPS = (("first_kernel_to_end_of_bake", "bakeMs"), ("refit", "refitMs"), ("quantise", "quantiseMs"), ("wide", "wideMs"))


def med(xs):
    return round(statistics.median(xs), 4)


def waved(pos, nrm, phase):
    box = float(np.max(pos.max(axis=0) - pos.min(axis=0)))
    k = 9.0 / box
    h = (0.03 * box * np.sin(k * pos[:, 0] + phase) * np.cos(k * pos[:, 2] - 0.5 * phase)).astype(np.float32)
    return (pos + nrm * h[:, None]).astype(np.float32)


def summary(walls, infos):
    groups = {name: med([i[key] for i in infos]) for name, key in GROUPS}
    inside = med([i["totalSeconds"] * 1e3 for i in infos])
    return {"wall_ms": med(walls), "wall_ms_all": [round(w, 4) for w in walls], "groups_ms": groups, "call_clock_ms": inside,
            "outside_the_call_clock_ms": round(med(walls) - inside, 4), "copies_and_synchronisation_ms": round(inside - sum(groups.values()), 4)}


def device_cost(pt, torch, dsc, scene_path, rounds, warmups):
    host = pt.HostScene.load(scene_path, os.path.join(ROOT, "scenes"))
    pos, nrm, tan, idx = dsc.mesh_data(host, 0)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True, deformable=True, primitives=True, vertex_normals=True)
    extra = () if tan is None else (tan,)
    d_nrm = torch.from_numpy(nrm).cuda()
    d_extra = tuple(torch.from_numpy(a).cuda() for a in extra)
    calls = {"host": lambda p, d: dev.set_mesh_vertices({0: (p, nrm) + extra}),
             "given": lambda p, d: dev.set_mesh_vertices_device({0: (d, d_nrm) + d_extra}),
             "computed": lambda p, d: dev.set_mesh_vertices_device({0: (d, None) + d_extra})}
    walls, infos = {k: [] for k in calls}, {k: [] for k in calls}
    for k in range(rounds + warmups):
        p = waved(pos, nrm, 0.3 * (k + 1))
        d = torch.from_numpy(p).cuda()
        torch.cuda.synchronize()
        for name, call in calls.items():
            t0 = time.perf_counter()
            info = call(p, d)
            if k >= warmups:
                walls[name].append((time.perf_counter() - t0) * 1e3)
                infos[name].append(info)
    dev.close()
    report = {"scene": os.path.relpath(scene_path, ROOT), "mesh_triangles": int(len(idx)), "mesh_vertices": int(len(pos)),
              "bytes_per_call_given": int(pos.nbytes + nrm.nbytes + sum(a.nbytes for a in extra)),
              "adjacency_bytes": int(len(idx) * 12 + (len(pos) + 1) * 4), "corner_table_bytes": int(len(idx) * 12)}
    for name in calls:
        report[name] = summary(walls[name], infos[name])
    bake = {name: report[name]["groups_ms"]["first_kernel_to_end_of_bake"] for name in calls}
    report["groups_by_difference_ms"] = {"gather_and_bake": bake["host"], "finiteness_kernel_read_back_and_synchronisation": round(bake["given"] - bake["host"], 4),
                                         "normals_kernel": round(bake["computed"] - bake["given"], 4)}
    report["given_over_host_wall"] = round(report["given"]["wall_ms"] / report["host"]["wall_ms"], 4)
    report["computed_over_host_wall"] = round(report["computed"]["wall_ms"] / report["host"]["wall_ms"], 4)
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_device_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import deform_scenes as dsc
    from scenes.gen_assets import ensure_assets, ensure_large_asset

    if pt.device_count() < 1:
        raise SystemExit("tools/dynamic_device_cost.py needs a GPU")
    ensure_assets()
    scenes = os.path.join(ROOT, "scenes")
    reports = []
    for name in ("cornell_mesh.scene", "knot_glass.scene"):
        path = os.path.join(scenes, name)
        with open(path) as f:
            for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
                ensure_large_asset(asset)
        reports.append(device_cost(pt, torch, dsc, path, args.rounds, args.warmups))
    report = {"timing": "wall time of the call and device events around its kernel groups; host-pointer, device-pointer with given normals and "
                        "device-pointer with computed normals take turns within a round; median of %d rounds after %d warm-ups" % (args.rounds, args.warmups),
              "scenes": reports}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
