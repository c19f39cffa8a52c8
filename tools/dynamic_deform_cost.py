#!/usr/bin/env python3
"""What deforming a mesh and moving a light of a dynamic scene (include/ptr_deform.h) cost, in one job on one GPU.

  deform   ptr_scene_set_mesh_vertices on the mesh of BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3]
           (scenes/knot_glass.scene): a sinusoidal displacement along the normals, the phase advanced per call.  The call's wall time and
           its kernel groups by device events (gather + bake, refit, quantise, wide), median of 5 after 2 warm-ups, against ptr_scene_upload
           of the description with the same vertex data.  Staging is its own line: the host pass that checks every component while copying
           it to the pinned buffer (wall time outside the call's own clock), and the host-to-device copy with the call's synchronisations
           (the call's clock minus its kernel groups), beside the bytes staged.
  light    ptr_scene_set_rects on the light rectangle of configs[1], likewise.
  quality  k_extend + k_connect kernel time per frame (1920x1080, depth 8, 16 spp) on the deformed, refitted tree over a fresh upload of
           the same vertex data.

  python tools/dynamic_deform_cost.py [--out profiles/dynamic_deform_cost.json]

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


def med(xs):
    return round(statistics.median(xs), 4)


def waved(pos, nrm, phase):
    box = float(np.max(pos.max(axis=0) - pos.min(axis=0)))
    k = 9.0 / box
    h = (0.03 * box * np.sin(k * pos[:, 0] + phase) * np.cos(k * pos[:, 2] - 0.5 * phase)).astype(np.float32)
    return (pos + nrm * h[:, None]).astype(np.float32)


def timed(call, states, warmups):
    walls, infos = [], []
    for k, state in enumerate(states):
        t0 = time.perf_counter()
        info = call(state)
        if k >= warmups:
            walls.append((time.perf_counter() - t0) * 1e3)
            infos.append(info)
    groups = {name: med([i[key] for i in infos]) for name, key in (("gather_bake", "bakeMs"), ("refit", "refitMs"), ("quantise", "quantiseMs"), ("wide", "wideMs"))}
    inside = med([i["totalSeconds"] * 1e3 for i in infos])
    return {"wall_ms": med(walls), "wall_ms_all": [round(w, 4) for w in walls], "groups_ms": groups, "call_clock_ms": inside,
            "host_staging_ms": round(med(walls) - inside, 4), "copy_and_synchronisation_ms": round(inside - sum(groups.values()), 4)}


def upload_ms(pt, holder, rounds):
    out = []
    for _ in range(min(rounds, 3)):
        t0 = time.perf_counter()
        fresh = pt.DeviceScene(holder.desc, 0, keepalive=holder)
        out.append((time.perf_counter() - t0) * 1e3)
        fresh.close()
    return med(out)


def deform_cost(pt, dsc, scene_path, rounds, warmups, quality):
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(scene_path, scenes)
    pos, nrm, tan, idx = dsc.mesh_data(host, 0)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True, deformable=True, primitives=True)
    extra = () if tan is None else (tan,)
    states = [(waved(pos, nrm, 0.3 * (k + 1)), nrm) + extra for k in range(rounds + warmups)]
    report = {"scene": os.path.relpath(scene_path, ROOT), "mesh_triangles": int(len(idx)), "mesh_vertices": int(len(pos)),
              "staged_bytes": int(sum(a.nbytes for a in states[0])), "corner_table_bytes": int(len(idx) * 12)}
    report["set_mesh_vertices"] = timed(lambda state: dev.set_mesh_vertices({0: state}), states, warmups)
    changed = dsc.Changed(host, vertices={0: states[-1]})
    report["upload_of_deformed_description_ms"] = upload_ms(pt, changed, rounds)
    report["upload_over_update"] = round(report["upload_of_deformed_description_ms"] / report["set_mesh_vertices"]["wall_ms"], 1)
    if host.desc.rectCount:
        diffuse_light = 3   # PTR_MAT_DIFFUSE_LIGHT
        lights = [i for i in range(host.desc.rectCount) if int(host.desc.materials[host.desc.rects[i].materialTwoSided[0]].typeEta[0]) == diffuse_light]
        if lights:
            r = dsc.rect_of(host, lights[0])
            moves = [dict(r, corner=r["corner"] + np.float32(3.0 * (k + 1)) * r["edgeU"] / np.float32(100.0)) for k in range(rounds + warmups)]
            report["light_rectangle"] = lights[0]
            report["set_rects"] = timed(lambda move: dev.set_rects({lights[0]: move}), moves, warmups)
            report["upload_over_set_rects"] = round(report["upload_of_deformed_description_ms"] / report["set_rects"]["wall_ms"], 1)
            dev.set_rects({lights[0]: r})
    if quality:
        s = host.settings_for(width=quality[0], height=quality[1], max_depth=8, seed=1337)
        fresh = pt.DeviceScene(changed.desc, 0, keepalive=changed)
        ms = {"refitted": [], "fresh": []}
        for k in range(4):   # alternating; the first pair warms up
            for name, scene in (("refitted", dev), ("fresh", fresh)):
                st = scene.render(s, quality[2])[1]
                if k:
                    ms[name].append(st.traceKernelMs + st.shadowKernelMs)
        fresh.close()
        a, b = statistics.median(ms["refitted"]), statistics.median(ms["fresh"])
        report["refit_quality"] = {"resolution": list(quality[:2]), "max_depth": 8, "spp": quality[2], "extend_connect_ms_refitted": round(a, 3),
                                   "extend_connect_ms_fresh": round(b, 3), "refitted_over_fresh": round(a / b, 4)}
    dev.close()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_deform_cost.json"), help="the report file")
    args = ap.parse_args()
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import deform_scenes as dsc
    from scenes.gen_assets import ensure_assets, ensure_large_asset

    ensure_assets()
    scenes = os.path.join(ROOT, "scenes")
    reports = []
    for name in ("cornell_mesh.scene", "knot_glass.scene"):
        path = os.path.join(scenes, name)
        with open(path) as f:
            for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
                ensure_large_asset(asset)
        reports.append(deform_cost(pt, dsc, path, args.rounds, args.warmups, (args.width, args.height, args.spp)))
    report = {"timing": "wall time of the call and device events around its kernel groups; median of %d after %d warm-ups; refit quality: k_extend + "
                        "k_connect kernel ms per frame (PtrRenderStats), median of 3 alternating frames after a warm-up" % (args.rounds, args.warmups),
              "scenes": reports}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
