#!/usr/bin/env python3
"""What temporal accumulation (include/ptr_temporal.h) costs and what it does to a sequence, in one process on one GPU.

Cost, at --width x --height (1920x1080) on BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3] (scenes/knot_glass.scene), each
uploaded dynamic: ptr_temporal_step_device on a device-resident frame, its three groups (k_surface, k_temporal_accumulate, the pose
snapshot) between device events, median of --rounds steps after --warmups; beside them ptr_render_aovs of the same frame (k_aovs plus its
two allocations and downloads, wall time) and, for the accumulate kernel, a MODEL of its traffic, not a measurement: every lane's own
bytes once, plus for the measured share of blending pixels four taps of 48 B requested, of which neighbouring lanes are taken to share
all but one; that modelled byte count over the measured time is given as a share of the HBM peak (the records were written by the
kernel before and may well sit in the last-level cache: the figure says the kernel is bound by bytes, not where they come from).
tools/denoise_bench.py --out profiles/denoise_1080p.json records one a-trous pass of the denoiser to put beside the accumulate time.

Sequence, on configs[1] at --seq-width x --seq-height: 16 frames, the mesh turned 2 degrees about y per frame, the camera's yaw drifting
0.2 degrees per frame, 4 spp per frame with a seed of its own.  Per frame the RMSE against a --reference-spp frame of the same pose of
the raw frame, the denoised frame (ptr_denoise alone), the accumulated frame (temporal alone) and the accumulated then denoised frame;
and per image kind the flicker: the mean absolute difference of consecutive frames minus that of the consecutive references.

  python tools/temporal_cost.py [--out profiles/temporal_cost.json]

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

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X HBM3E, specified peak
# k_temporal_accumulate per pixel, each byte once: rgb in, three records, out rgb, length, history out; and per blended pixel the taps'
# history and two records, which neighbouring lanes share: one more pixel's worth when the motion is smooth
OWN_BYTES, TAP_BYTES = 12 + 48 + 12 + 4 + 16, 48


def med(xs):
    return round(statistics.median(xs), 4)


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)


def load(pt, name):
    from scenes.gen_assets import ensure_large_asset

    scenes = os.path.join(ROOT, "scenes")
    path = os.path.join(scenes, name)
    with open(path) as f:
        for asset in re.findall(r"assets/(\w+_\d{6,}\.ply)", f.read()):
            ensure_large_asset(asset)
    return pt.HostScene.load(path, scenes)


def step_cost(pt, torch, name, width, height, rounds, warmups):
    host = load(pt, name)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    s = host.settings_for(width=width, height=height, max_depth=8, seed=1337)
    frame = torch.from_numpy(dev.render_image(s, 4)[0]).cuda()
    out, length = torch.empty_like(frame), torch.empty((height, width), dtype=torch.float32, device="cuda:0")
    albedo, normal = (torch.empty((height, width, 4), dtype=torch.float32, device="cuda:0") for _ in range(2))
    temporal = dev.temporal(width, height)
    infos, walls, aov_walls = [], [], []
    for k in range(rounds + warmups):
        s.seed = 2000 + k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = temporal.step_device(s, frame, out, length, albedo, normal, want_info=True)
        wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dev.render_aovs(s, 0)
        aov_wall = (time.perf_counter() - t0) * 1e3
        if k >= warmups:
            infos.append(info)
            walls.append(wall)
            aov_walls.append(aov_wall)
    blended = float((length > 1.0).float().mean().item())
    temporal.close()
    info = dev.info()
    dev.close()
    pixels = width * height
    accumulate = med([i["accumulateMs"] for i in infos])
    least = pixels * (OWN_BYTES + blended * TAP_BYTES)
    requested = pixels * (OWN_BYTES + blended * 4 * TAP_BYTES)
    return {"scene": "scenes/" + name, "width": width, "height": height, "triangles": info["triangles"], "spheres": info["spheres"],
            "surface_ms": med([i["surfaceMs"] for i in infos]), "accumulate_ms": accumulate, "snapshot_ms": med([i["snapshotMs"] for i in infos]),
            "snapshot_bytes": info["triangles"] * 48 + info["spheres"] * 16, "step_wall_ms": med(walls),
            "render_aovs_wall_ms_with_its_downloads": med(aov_walls), "blended_pixel_share": round(blended, 4),
            "accumulate_bytes_requested_modelled": int(requested), "accumulate_bytes_distinct_modelled": int(least),
            "accumulate_modelled_bytes_over_time_share_of_hbm_peak": round(least / (accumulate * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if accumulate > 0 else None}


def sequence(pt, width, height, frames, spp, reference_spp):
    from test_gpu_dynamic import matrix_of

    host = load(pt, "cornell_mesh.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    temporal = dev.temporal(width, height)
    base = matrix_of(host, 0).astype(np.float64)
    kinds = ("raw", "denoise", "temporal", "temporal_denoise")
    images = {k: [] for k in kinds}
    references, rows = [], []
    rmse = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))
    for k in range(frames):
        s = host.settings_for(width=width, height=height, max_depth=8, seed=3000 + k)
        s.cameraYaw += float(np.radians(0.2) * k)
        dev.set_mesh_transforms({0: (base @ rotation_y(np.radians(2.0) * k)).astype(np.float32)})
        raw = dev.render_image(s, spp)[0]
        ref_settings = s.copy()
        ref_settings.seed = 9000 + k
        references.append(dev.render_image(ref_settings, reference_spp)[0])
        step = temporal.step(s, raw, want_aovs=True)
        images["raw"].append(raw)
        images["denoise"].append(pt.denoise(raw, step["albedo"], step["normal"]))
        images["temporal"].append(step["rgb"])
        images["temporal_denoise"].append(pt.denoise(step["rgb"], step["albedo"], step["normal"]))
        rows.append({"frame": k, "mean_history_length": round(float(step["length"].mean()), 3),
                     **{"rmse_" + kind: round(rmse(images[kind][-1], references[-1]), 5) for kind in kinds}})
    temporal.close()
    dev.close()
    between = lambda seq: float(np.mean([np.mean(np.abs(a.astype(np.float64) - b.astype(np.float64))) for a, b in zip(seq[1:], seq[:-1])]))
    floor = between(references)
    return {"scene": "scenes/cornell_mesh.scene", "width": width, "height": height, "frames": frames, "spp": spp, "reference_spp": reference_spp,
            "mesh_turn_degrees_per_frame": 2.0, "yaw_drift_degrees_per_frame": 0.2, "per_frame": rows,
            "mean_abs_difference_of_consecutive_references": round(floor, 6),
            "flicker": {kind: round(between(images[kind]) - floor, 6) for kind in kinds},
            "mean_rmse": {kind: round(float(np.mean([r["rmse_" + kind] for r in rows])), 5) for kind in kinds}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--seq-width", type=int, default=960)
    ap.add_argument("--seq-height", type=int, default=540)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    from scenes.gen_assets import ensure_assets

    if pt.device_count() < 1:
        raise SystemExit("tools/temporal_cost.py needs a GPU")
    ensure_assets()
    report = {"timing": "device events around the three groups of ptr_temporal_step_device on a device-resident frame, median of %d steps "
                        "after %d warm-ups; wall time around the call" % (args.rounds, args.warmups),
              "steps": [step_cost(pt, torch, name, args.width, args.height, args.rounds, args.warmups)
                        for name in ("cornell_mesh.scene", "knot_glass.scene")],
              "sequence": sequence(pt, args.seq_width, args.seq_height, args.frames, args.spp, args.reference_spp)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
