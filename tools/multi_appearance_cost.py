#!/usr/bin/env python3
"""What an appearance update costs on a frame on several devices (include/ptr_multi_appearance.h), in one job on one GPU.

On BASELINE configs[1] (scenes/cornell_mesh.scene: materials) and configs[2] (scenes/helmet_env.scene: its environment map), and on one
1024 x 1024 texture (a quad built in memory, tests/appearance_scenes.Quads: neither config carries a texture of that size), at 1920x1080,
with ONE partition ([0]) and with TWO partitions on the same device ([0, 0]):

  materials     a colour edit (no type change), a type change that rekeys every triangle row, the light dimmed
  textures      the 1024 x 1024 texture from host pixels and from a tensor on device 0
  environment   the config's map from host pixels and from a tensor on device 0

Per case: the wall time of the MultiFrame call beside the wall time of the same call on a single-device DeviceScene, measured in the same
run and in turns (one call on the scene, one on the frame, and again); distributeSeconds, partSeconds and hostStagedBytes of
PtrMultiAppearanceInfo.  Median of 5 after 2 warm-ups.  Beside them: multi_frame() of the edited description, which is what the edit
cost before.

Everything here runs on ONE device: repeated ids put every partition on the same GPU, which measures the protocol - threads, the one
staging, the event - and nothing about scaling over real devices, which is unmeasured.

  python tools/multi_appearance_cost.py [--out profiles/multi_appearance_cost.json]

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LISTS = ([0], [0, 0])


def med(xs):
    return round(statistics.median(xs), 4)


def in_turns(single, multi, states, warmups):
    """single(state) on the DeviceScene, then multi(state) on the MultiFrame, state after state."""
    walls = {"single": [], "multi": []}
    infos = []
    for k, state in enumerate(states):
        for name, call in (("single", single), ("multi", multi)):
            t0 = time.perf_counter()
            info = call(state)
            wall = (time.perf_counter() - t0) * 1e3
            if k >= warmups:
                walls[name].append(wall)
                if name == "multi":
                    infos.append(info)
    return {"single_device_wall_ms": med(walls["single"]), "wall_ms": med(walls["multi"]), "wall_ms_all": [round(w, 4) for w in walls["multi"]],
            "call_ms": med([i["totalSeconds"] * 1e3 for i in infos]), "distribute_ms": med([i["distributeSeconds"] * 1e3 for i in infos]),
            "part_ms": [med([i["partSeconds"][p] * 1e3 for i in infos]) for p in range(infos[-1]["parts"])],
            "hostStagedBytes": infos[-1]["hostStagedBytes"], "stagedParts": infos[-1]["stagedParts"],
            "first_partition_steps_ms": [med([i["kernelMs"][g] for i in infos]) for g in range(6)]}


def create_ms(pt, holder, s, ids, **flags):
    """multi_frame() of holder.desc (the holder keeps the description's arrays alive)."""
    desc = holder.desc
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        frame = pt.multi_frame(desc, s, device_ids=ids, **flags)
        out.append((time.perf_counter() - t0) * 1e3)
        frame.close()
    return med(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_appearance_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import appearance_scenes as aps
    from scenes.gen_assets import ensure_assets

    if pt.device_count() < 1:
        raise SystemExit("tools/multi_appearance_cost.py needs a GPU")
    ensure_assets()
    n = args.rounds + args.warmups
    scenes = os.path.join(ROOT, "scenes")
    dyn = dict(dynamic=True, primitives=True)
    size = dict(width=args.width, height=args.height, max_depth=8, seed=1337)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    report = {"timing": "wall ms of the call (time.perf_counter around it) on a MultiFrame beside the same call on a single-device DeviceScene, in turns in "
                        "one run; call_ms, distribute_ms and part_ms are totalSeconds, distributeSeconds and partSeconds of PtrMultiAppearanceInfo; median "
                        "of %d after %d warm-ups; %dx%d" % (args.rounds, args.warmups, args.width, args.height),
              "visible_devices": pt.device_count(),
              "measured_on": "ONE device: the lists [0] and [0, 0] put every partition on the same GPU",
              "scaling_over_real_devices": "unmeasured"}

    # ---- materials, config 2
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    d = host.desc
    s = host.settings_for(**size)
    mesh_material = d.meshes[0].materialIndex
    was = int(d.materials[mesh_material].typeEta[0])
    light = next(i for i in range(d.materialCount) if int(d.materials[i].typeEta[0]) == 3)
    colours = [{mesh_material: aps.material_of(d, mesh_material, baseColorRoughness=(0.1 + 0.1 * k, 0.5, 0.3))} for k in range(n)]
    types = [{mesh_material: aps.material_of(d, mesh_material, typeEta=(float(1 - was if k % 2 == 0 else was),))} for k in range(n)]
    dimmed = [{light: aps.material_of(d, light, emission=(10.0 - k, 8.0, 6.0))} for k in range(n)]
    report["materials"] = {"scene": "scenes/cornell_mesh.scene"}
    for ids in LISTS:
        dev = pt.DeviceScene(d, 0, keepalive=host, **dyn)
        frame = pt.multi_frame(d, s, device_ids=ids, **dyn)
        report["materials"]["triangles"] = dev.info()["triangles"]
        report["materials"]["-".join(map(str, ids))] = {
            "colour_only": in_turns(dev.set_materials, frame.set_materials, colours, args.warmups),
            "type_change_that_rekeys": in_turns(dev.set_materials, frame.set_materials, types, args.warmups),
            "light_dimmed": in_turns(dev.set_materials, frame.set_materials, dimmed, args.warmups),
            "multi_frame_create_of_the_edited_description_ms": create_ms(pt, aps.Edited(d, host, materials=dimmed[-1]), s, ids, **dyn)}
        frame.close()
        dev.close()

    # ---- one 1024 x 1024 texture
    quads = aps.Quads(((1024, 1024),))
    d = quads.desc
    s = quads.settings(s, True)
    s.width, s.height = args.width, args.height
    rng = np.random.default_rng(1)
    pixels = [rng.random((1024, 1024, 4), dtype=np.float32) for _ in range(2)]
    tensors = [on(p) for p in pixels]
    torch.cuda.synchronize(0)
    report["textures"] = {"scene": "one quad under a 1024 x 1024 texture (tests/appearance_scenes.Quads)", "bytes": int(pixels[0].nbytes)}
    for ids in LISTS:
        dev = pt.DeviceScene(d, 0, keepalive=quads)
        frame = pt.multi_frame(d, s, device_ids=ids)
        report["textures"]["-".join(map(str, ids))] = {
            "from_host_pixels": in_turns(lambda k: dev.set_textures({0: pixels[k % 2]}), lambda k: frame.set_textures({0: pixels[k % 2]}), list(range(n)), args.warmups),
            "from_device_pixels": in_turns(lambda k: dev.set_textures_device({0: tensors[k % 2]}), lambda k: frame.set_textures_device({0: tensors[k % 2]}), list(range(n)),
                                           args.warmups),
            "multi_frame_create_of_the_edited_description_ms": create_ms(pt, aps.Edited(d, quads, textures={0: pixels[1]}), s, ids)}
        frame.close()
        dev.close()

    # ---- environment, config 3
    host = pt.HostScene.load(os.path.join(scenes, "helmet_env.scene"), scenes)
    d = host.desc
    s = host.settings_for(**size)
    w, h = d.envWidth, d.envHeight
    own = np.ctypeslib.as_array(d.envRgba, shape=(h, w, 4)).copy()
    maps = [np.ascontiguousarray(np.roll(own, 37 * (k + 1), axis=1)) for k in range(2)]
    tensors = [on(m) for m in maps]
    torch.cuda.synchronize(0)
    report["environment"] = {"scene": "scenes/helmet_env.scene", "size": [w, h], "bytes": int(maps[0].nbytes),
                             "first_partition_steps": ["pixels_and_check", "weights_and_row_sums", "sequential_total", "alias_tables", "pdf", "mip_chain"]}
    for ids in LISTS:
        dev = pt.DeviceScene(d, 0, keepalive=host)
        frame = pt.multi_frame(d, s, device_ids=ids)
        report["environment"]["-".join(map(str, ids))] = {
            "from_host_pixels": in_turns(lambda k: dev.set_environment(maps[k % 2]), lambda k: frame.set_environment(maps[k % 2]), list(range(n)), args.warmups),
            "from_device_pixels": in_turns(lambda k: dev.set_environment_device(tensors[k % 2]), lambda k: frame.set_environment_device(tensors[k % 2]), list(range(n)),
                                           args.warmups),
            "multi_frame_create_of_the_edited_description_ms": create_ms(pt, aps.Edited(d, host, env=maps[1]), s, ids)}
        frame.close()
        dev.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
