#!/usr/bin/env python3
"""What an in-place update of a dynamic scene costs on a frame on several devices (include/ptr_multi_dynamic.h), in one job.

On BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3] (scenes/knot_glass.scene) at 1920x1080, median of 5 after 2 warm-ups:
  per P   for P in 1, 2, 4, 8 real devices (as many as the machine has): the wall time of MultiFrame.set_mesh_transforms,
          set_mesh_vertices, set_mesh_vertices_device (given and computed normals, the arrays on device 0) and rebuild_tree, with
          distributeSeconds and the slowest partSeconds of PtrMultiUpdateInfo; and multi_frame() of the moved description, static: what
          a caller paid per pose before.
  single  the same calls on a single-device DeviceScene in the same run.
  protocol  on a machine with ONE device: the lists [0, 0] and [0, -1] (repeated ids; the second partition forced through pinned host
          memory).  They measure the protocol - threads, the event, the staging copy - and say nothing about scaling: the report's
          `scaling` rows stay empty there.

  python tools/multi_dynamic_cost.py [--out profiles/multi_dynamic_cost.json]

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

FLAGS = dict(dynamic=True, deformable=True, vertex_normals=True)


def med(xs):
    return round(statistics.median(xs), 4)


def timed(call, rounds, warmups, before=None):
    """Median wall ms of call(k) as Python sees it; call_ms, the library's own totalSeconds of an update call (PtrUpdateInfo's on a
    DeviceScene, PtrMultiUpdateInfo's on a MultiFrame: without the marshalling of the arguments); and, on a MultiFrame, distributeSeconds
    and the slowest partSeconds."""
    walls, inside, spread, slowest = [], [], [], []
    for k in range(rounds + warmups):
        if before:
            before(k)
        t0 = time.perf_counter()
        info = call(k)
        wall = (time.perf_counter() - t0) * 1e3
        if k < warmups:
            continue
        walls.append(wall)
        if isinstance(info, dict) and "bakeMs" in info:
            inside.append(info["totalSeconds"] * 1e3)
        if isinstance(info, dict) and "distributeSeconds" in info:
            spread.append(info["distributeSeconds"] * 1e3)
            slowest.append(max(info["partSeconds"]) * 1e3)
    out = {"wall_ms": med(walls)}
    if inside:
        out["call_ms"] = med(inside)
    if spread:
        out.update(distribute_ms=med(spread), slowest_part_ms=med(slowest))
    return out


def calls_on(target, torch, host, dsc, rounds, warmups):
    """The five calls on `target`, a MultiFrame or a DeviceScene."""
    pos, nrm, tan, _ = dsc.mesh_data(host, 0)
    poses = []
    for k in range(rounds + warmups):
        moved = (pos + np.float32(0.001 * (k + 1)) * nrm).astype(np.float32)
        poses.append((moved, nrm) if tan is None else (moved, nrm, tan))
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    given = [tuple(on(a) for a in p) for p in poses]
    computed = [(g[0], None) + g[2:] for g in given]
    turns = [turned(host, 5.0 + k) for k in range(rounds + warmups)]
    torch.cuda.synchronize(0)
    out = {"set_mesh_transforms": timed(lambda k: target.set_mesh_transforms({0: turns[k]}), rounds, warmups),
           "set_mesh_vertices": timed(lambda k: target.set_mesh_vertices({0: poses[k]}), rounds, warmups),
           "set_mesh_vertices_device": timed(lambda k: target.set_mesh_vertices_device({0: given[k]}), rounds, warmups),
           "set_mesh_vertices_device_computed_normals": timed(lambda k: target.set_mesh_vertices_device({0: computed[k]}), rounds, warmups),
           "rebuild_tree": timed(lambda k: target.rebuild_tree(keep_if_better=False), rounds, warmups,
                                 before=lambda k: target.set_mesh_transforms({0: turned(host, 45.0 + k)}))}
    out["vertex_bytes"] = int(sum(a.nbytes for a in poses[0]))
    return out


def one_list(pt, torch, dsc, host, s, ids, rounds, warmups):
    frame = pt.multi_frame(host.desc, s, device_ids=ids, **FLAGS)
    try:
        report = calls_on(frame, torch, host, dsc, rounds, warmups)
    finally:
        frame.close()
    moved = dsc.Changed(host, matrices={0: turned(host, 45.0)})
    creates = []
    for _ in range(3):
        t0 = time.perf_counter()
        static = pt.multi_frame(moved.desc, s, device_ids=ids)
        creates.append((time.perf_counter() - t0) * 1e3)
        static.close()
    report["multi_frame_create_of_the_moved_description_ms"] = med(creates)
    report["device_ids"] = ids
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_dynamic_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import deform_scenes as dsc
    from scenes.gen_assets import ensure_assets, ensure_large_asset

    devices = pt.device_count()
    if devices < 1:
        raise SystemExit("tools/multi_dynamic_cost.py needs a GPU")
    ensure_assets()
    scenes = os.path.join(ROOT, "scenes")
    reports = []
    for name in ("cornell_mesh.scene", "knot_glass.scene"):
        path = os.path.join(scenes, name)
        with open(path) as f:
            for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
                ensure_large_asset(asset)
        host = pt.HostScene.load(path, scenes)
        s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
        single = pt.DeviceScene(host.desc, 0, keepalive=host, **FLAGS)
        try:
            report = {"scene": os.path.relpath(path, ROOT), "single_device": calls_on(single, torch, host, dsc, args.rounds, args.warmups)}
        finally:
            single.close()
        report["scaling"] = {"P=%d" % p: one_list(pt, torch, dsc, host, s, list(range(p)), args.rounds, args.warmups) for p in (1, 2, 4, 8) if p <= devices}
        if devices == 1:
            del report["scaling"]["P=1"]["device_ids"]
            report["one_partition"] = report["scaling"].pop("P=1")
            report["protocol_on_one_device"] = {"-".join(map(str, ids)): one_list(pt, torch, dsc, host, s, ids, args.rounds, args.warmups)
                                                for ids in ([0, 0], [0, -1], [0, 0, 0, 0])}
        reports.append(report)
    report = {"timing": "wall ms of the call (time.perf_counter around it), distributeSeconds and the slowest partSeconds of PtrMultiUpdateInfo; median of "
                        "%d after %d warm-ups; %dx%d" % (args.rounds, args.warmups, args.width, args.height),
              "visible_devices": devices,
              "scaling_measured": devices > 1,
              "note": "with one visible device `scaling` is empty: repeated ids run every partition on the same GPU, which measures the protocol "
                      "(threads, the event, the staging copy) and nothing about scaling" if devices == 1 else "",
              "scenes": reports}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
