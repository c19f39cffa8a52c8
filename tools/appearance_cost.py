#!/usr/bin/env python3
"""What changing the appearance of a resident scene (include/ptr_appearance.h) costs, in one job on one GPU.

  materials    ptr_scene_set_materials on BASELINE configs[1] (scenes/cornell_mesh.scene, uploaded with PTR_DYNAMIC_PRIMITIVES): the mesh's
               material with another colour (no type change), the same material from Lambert to metal and back (the rekey kernel runs over
               every triangle row), and the emission of the light.
  textures     ptr_scene_set_textures / ptr_scene_set_textures_device on the largest texture of the repository's textured glTF
               (tests/golden/textured.scene).
  environment  ptr_scene_set_environment / ptr_scene_set_environment_device on the map of configs[2], with the sequential total
               (k_app_env_total) and the alias tables (k_app_env_alias) apart, beside the seconds the upload's host build of the shading
               tables took (ptr_scene_timings).

Each figure is the median of 5 calls after 2 warm-ups, and stands against ptr_scene_upload_dynamic_ex of the edited description timed in
the same run.

  python tools/appearance_cost.py [--out profiles/appearance_cost.json]

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


def med(xs):
    return round(statistics.median(xs), 4)


def timed(call, states, warmups, names):
    walls, infos = [], []
    for k, state in enumerate(states):
        t0 = time.perf_counter()
        info = call(state)
        if k >= warmups:
            walls.append((time.perf_counter() - t0) * 1e3)
            infos.append(info)
    out = {"wall_ms": med(walls), "wall_ms_all": [round(w, 4) for w in walls], "call_clock_ms": med([i["totalSeconds"] * 1e3 for i in infos]),
           "staging_ms": med([i["stagingMs"] for i in infos])}
    out["steps_ms"] = {name: med([i["kernelMs"][k] for i in infos]) for k, name in enumerate(names)}
    for key in ("rowsRekeyed", "texelsWritten", "lightsAfter", "envSampling"):
        out[key] = int(infos[-1][key])
    return out


def upload_ms(pt, holder, rounds, **flags):
    out, tables = [], []
    for _ in range(min(rounds, 3)):
        t0 = time.perf_counter()
        fresh = pt.DeviceScene(holder.desc, 0, keepalive=holder, **flags)
        out.append((time.perf_counter() - t0) * 1e3)
        tables.append(fresh.timings()["shading_tables_s"] * 1e3)
        fresh.close()
    return {"upload_ms": med(out), "of_which_shading_tables_on_the_host_ms": med(tables)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    args = ap.parse_args()
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import appearance_scenes as aps
    import torch
    from scenes.gen_assets import ensure_assets

    ensure_assets()
    n = args.rounds + args.warmups
    scenes = os.path.join(ROOT, "scenes")
    dyn = dict(dynamic=True, primitives=True)
    report = {}

    # ---- materials, config 2
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    d = host.desc
    mesh_material = d.meshes[0].materialIndex
    light = next(i for i in range(d.materialCount) if int(d.materials[i].typeEta[0]) == 3)
    dev = pt.DeviceScene(d, 0, keepalive=host, **dyn)
    colours = [aps.material_of(d, mesh_material, baseColorRoughness=(0.1 + 0.1 * k, 0.5, 0.3)) for k in range(n)]
    types = [aps.material_of(d, mesh_material, typeEta=(float(1 - int(d.materials[mesh_material].typeEta[0]) if k % 2 == 0 else int(d.materials[mesh_material].typeEta[0])),))
             for k in range(n)]
    emissions = [aps.material_of(d, light, emission=(10.0 - k, 8.0, 6.0)) for k in range(n)]
    names = ("copies", "rekey")
    report["materials"] = {
        "scene": "scenes/cornell_mesh.scene", "triangles": dev.info()["triangles"],
        "colour_only": timed(lambda m: dev.set_materials({mesh_material: m}), colours, args.warmups, names),
        "type_change": timed(lambda m: dev.set_materials({mesh_material: m}), types, args.warmups, names),
        "light_emission": timed(lambda m: dev.set_materials({light: m}), emissions, args.warmups, names),
    }
    report["materials"].update(upload_ms(pt, aps.Edited(d, host, materials={light: emissions[-1]}), args.rounds, **dyn))
    dev.close()

    # ---- textures: the textured glTF of the repository (tests/golden/textured.scene; the stand-in of configs[2] carries no textures)
    golden = os.path.join(ROOT, "tests", "golden")
    host = pt.HostScene.load(os.path.join(golden, "textured.scene"), golden)
    d = host.desc
    dev = pt.DeviceScene(d, 0, keepalive=host, **dyn)
    t = max(range(d.textureCount), key=lambda i: d.textures[i].width * d.textures[i].height)
    tex = d.textures[t]
    rng = np.random.default_rng(1)
    pixels = [rng.random((tex.height, tex.width, 4), dtype=np.float32) for _ in range(2)]
    value = lambda a: (a, tex.wrapS, tex.wrapT, tex.filter)
    tensors = [torch.from_numpy(p).cuda() for p in pixels]
    names = ("copies_and_check", "mip_chain")
    report["textures"] = {
        "scene": "tests/golden/textured.scene", "texture": t, "size": [tex.width, tex.height],
        "from_host_pixels": timed(lambda k: dev.set_textures({t: value(pixels[k % 2])}), list(range(n)), args.warmups, names),
        "from_device_pixels": timed(lambda k: dev.set_textures_device({t: value(tensors[k % 2])}), list(range(n)), args.warmups, names),
    }
    report["textures"].update(upload_ms(pt, aps.Edited(d, host, textures={t: value(pixels[1])}), args.rounds, **dyn))
    dev.close()

    # ---- environment, config 3
    host = pt.HostScene.load(os.path.join(scenes, "helmet_env.scene"), scenes)
    d = host.desc
    dev = pt.DeviceScene(d, 0, keepalive=host, **dyn)
    w, h = d.envWidth, d.envHeight
    own = np.ctypeslib.as_array(d.envRgba, shape=(h, w, 4)).copy()
    maps = [np.ascontiguousarray(np.roll(own, 37 * (k + 1), axis=1)) for k in range(2)]
    tensors = [torch.from_numpy(m).cuda() for m in maps]
    names = ("pixels_and_check", "weights_and_row_sums", "sequential_total", "alias_tables", "pdf", "mip_chain")
    report["environment"] = {
        "scene": "scenes/helmet_env.scene", "size": [w, h],
        "from_host_pixels": timed(lambda k: dev.set_environment(maps[k % 2]), list(range(n)), args.warmups, names),
        "from_device_pixels": timed(lambda k: dev.set_environment_device(tensors[k % 2]), list(range(n)), args.warmups, names),
    }
    report["environment"].update(upload_ms(pt, aps.Edited(d, host, env=maps[1]), args.rounds, **dyn))
    dev.close()

    text = json.dumps(report)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(text)


if __name__ == "__main__":
    main()
