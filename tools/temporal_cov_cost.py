#!/usr/bin/env python3
"""What carrying the covariance through temporal accumulation (include/ptr_temporal_cov.h) costs and what it is worth, in one process on
one GPU.  Everything here is a measurement to be recorded; none is a condition of any test.

(a) kernel: at --width x --height (1920x1080) on BASELINE configs[1] (scenes/cornell_mesh.scene) and configs[3]
    (scenes/knot_glass.scene), each uploaded dynamic, k_temporal_accumulate_cov against k_temporal_accumulate in the same job: the
    accumulate group of ptr_temporal_step_cov_device and of ptr_temporal_step_device between device events, the two handles stepped in
    turn on the same device-resident 4-spp frame, median of --rounds steps after --warmups.
(b) turntable: tools/temporal_cost.py's sequence (configs[1], --seq-width x --seq-height, 16 frames, the mesh turned 2 degrees and the
    camera's yaw drifting 0.2 degrees per frame, 4 spp, --reference-spp references).  RMSE and flicker of four pipelines:
      temporal_denoise            temporal, then ptr_denoise (the 7x7 spatial variance estimate)
      temporal_cov_denoise_cov    temporal-cov, then ptr_denoise_cov on the PROPAGATED covariance
      temporal_cov0_denoise_cov   the same with rejectSigma 0: the propagation without the consistency test
      temporal_denoise_frame_cov  temporal, then ptr_denoise_cov on the frame's OWN covariance: the mis-scaled input
(c) calibration: a static pose of configs[1]; at frames 1, 4 and 16, over the hit pixels, the mean squared luminance error of the
    accumulated frame against the reference over the mean of lumvar(out_cov).  Near 1 if the propagation is right.
(d) a moved light: configs[1] with its light rectangle sliding --light-step units along x per frame (ptr_scene_set_rects), a reference per
    frame.  RMSE with rejectSigma 0 and 3 inside the region whose reference changes (luminance differing from the previous frame's
    reference by more than 5 % of the frame's mean luminance) and outside it; and on the static sequence of (c) the share of hit pixels with
    a history that the consistency test rejects per frame: the false-rejection rate at 4 spp.

  python tools/temporal_cov_cost.py [--out profiles/temporal_cov_cost.json]

Needs a GPU (no CPU fallback).  The report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from temporal_cost import load, med, rotation_y   # noqa: E402

K = np.array([0.2126, 0.7152, 0.0722])
LIGHT_RECT = 5   # of scenes/cornell_mesh.scene


def lum(x):
    return x.astype(np.float64) @ K


def lumvar(c6):
    c = c6.astype(np.float64)
    diag = c[..., 0] * K[0] ** 2 + c[..., 1] * K[1] ** 2 + c[..., 2] * K[2] ** 2
    return np.maximum(diag + 2.0 * (c[..., 3] * K[0] * K[1] + c[..., 4] * K[0] * K[2] + c[..., 5] * K[1] * K[2]), 0.0)


def rmse(a, b, mask=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask]))) if mask is None or mask.any() else None


def between(seq):
    return float(np.mean([np.mean(np.abs(a.astype(np.float64) - b.astype(np.float64))) for a, b in zip(seq[1:], seq[:-1])]))


def kernel_cost(pt, torch, name, width, height, rounds, warmups):
    host = load(pt, name)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    s = host.settings_for(width=width, height=height, max_depth=8, seed=1337)
    rgb, cov, _ = dev.render_image_cov(s, 4)
    d_rgb, d_cov = torch.from_numpy(rgb).cuda(), torch.from_numpy(cov).cuda()
    out, out_cov = torch.empty_like(d_rgb), torch.empty_like(d_cov)
    length = torch.empty((height, width), dtype=torch.float32, device="cuda:0")
    plain, carrying = dev.temporal(width, height), dev.temporal(width, height, cov=True)
    ms = {"plain": [], "cov": []}
    for k in range(rounds + warmups):
        s.seed = 2000 + k
        a = plain.step_device(s, d_rgb, out, length, want_info=True)
        b = carrying.step_device(s, d_rgb, out, length, want_info=True, cov=d_cov, out_cov=out_cov)
        if k >= warmups:
            ms["plain"].append(a["accumulateMs"])
            ms["cov"].append(b["accumulateMs"])
    blended = float((length > 1.0).float().mean().item())
    for t in (plain, carrying):
        t.close()
    dev.close()
    return {"scene": "scenes/" + name, "width": width, "height": height, "k_temporal_accumulate_ms": med(ms["plain"]),
            "k_temporal_accumulate_cov_ms": med(ms["cov"]), "ratio": round(med(ms["cov"]) / med(ms["plain"]), 3) if med(ms["plain"]) > 0 else None,
            "blended_pixel_share_cov": round(blended, 4), "own_bytes_per_lane": {"plain": 92, "cov": 164}, "tap_bytes": {"plain": 48, "cov": 72}}


def turntable(pt, width, height, frames, spp, reference_spp):
    from test_gpu_dynamic import matrix_of

    host = load(pt, "cornell_mesh.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    plain, carrying = dev.temporal(width, height), dev.temporal(width, height, cov=True)
    carrying0 = dev.temporal(width, height, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=0.0))
    base = matrix_of(host, 0).astype(np.float64)
    kinds = ("temporal_denoise", "temporal_cov_denoise_cov", "temporal_cov0_denoise_cov", "temporal_denoise_frame_cov")
    images = {k: [] for k in kinds}
    references, rows = [], []
    for k in range(frames):
        s = host.settings_for(width=width, height=height, max_depth=8, seed=3000 + k)
        s.cameraYaw += float(np.radians(0.2) * k)
        dev.set_mesh_transforms({0: (base @ rotation_y(np.radians(2.0) * k)).astype(np.float32)})
        raw, cov, _ = dev.render_image_cov(s, spp)
        ref_settings = s.copy()
        ref_settings.seed = 9000 + k
        references.append(dev.render_image(ref_settings, reference_spp)[0])
        a = plain.step(s, raw, want_aovs=True)
        b = carrying.step(s, raw, cov)
        b0 = carrying0.step(s, raw, cov)
        images["temporal_denoise"].append(pt.denoise(a["rgb"], a["albedo"], a["normal"]))
        images["temporal_cov_denoise_cov"].append(pt.denoise(b["rgb"], a["albedo"], a["normal"], cov=b["cov"]))
        images["temporal_cov0_denoise_cov"].append(pt.denoise(b0["rgb"], a["albedo"], a["normal"], cov=b0["cov"]))
        images["temporal_denoise_frame_cov"].append(pt.denoise(a["rgb"], a["albedo"], a["normal"], cov=cov))
        rows.append({"frame": k, "mean_history_length": round(float(a["length"].mean()), 3),
                     "mean_history_length_cov": round(float(b["length"].mean()), 3),
                     **{"rmse_" + kind: round(rmse(images[kind][-1], references[-1]), 5) for kind in kinds}})
    for t in (plain, carrying, carrying0):
        t.close()
    dev.close()
    floor = between(references)
    return {"scene": "scenes/cornell_mesh.scene", "width": width, "height": height, "frames": frames, "spp": spp, "reference_spp": reference_spp,
            "mesh_turn_degrees_per_frame": 2.0, "yaw_drift_degrees_per_frame": 0.2,
            "reject_sigma": {"temporal_cov_denoise_cov": 3.0, "temporal_cov0_denoise_cov": 0.0}, "per_frame": rows,
            "mean_abs_difference_of_consecutive_references": round(floor, 6),
            "flicker": {kind: round(between(images[kind]) - floor, 6) for kind in kinds},
            "mean_rmse": {kind: round(float(np.mean([r["rmse_" + kind] for r in rows])), 5) for kind in kinds}}


def static_pose(pt, width, height, frames, spp, reference_spp):
    """(c) and the second half of (d)."""
    host = load(pt, "cornell_mesh.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=width, height=height, max_depth=8, seed=9500)
    reference = dev.render_image(s, reference_spp)[0]
    handles = {3.0: dev.temporal(width, height, cov=True), 0.0: dev.temporal(width, height, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=0.0))}
    calibration, rejected = {sigma: [] for sigma in handles}, []
    for k in range(frames):
        s.seed = 5000 + k
        raw, cov, _ = dev.render_image_cov(s, spp)
        outs = {sigma: t.step(s, raw, cov) for sigma, t in handles.items()}
        had = outs[0.0]["length"] > 1   # hit pixels that found a history: what the consistency test looks at
        if k:
            rejected.append({"frame": k + 1, "share_of_hit_pixels_with_history_rejected":
                             round(float(((outs[3.0]["length"] == 1) & had).sum() / max(int(had.sum()), 1)), 5)})
        if k + 1 in (1, 4, 16):
            for sigma, out in outs.items():
                hit = out["length"] > 0
                error = float(np.mean((lum(out["rgb"]) - lum(reference))[hit] ** 2))
                predicted = float(np.mean(lumvar(out["cov"])[hit]))
                calibration[sigma].append({"frame": k + 1, "mean_squared_luminance_error": error, "mean_lumvar_of_out_cov": predicted,
                                           "ratio": round(error / predicted, 4) if predicted > 0 else None})
    for t in handles.values():
        t.close()
    dev.close()
    return {"scene": "scenes/cornell_mesh.scene", "width": width, "height": height, "frames": frames, "spp": spp, "reference_spp": reference_spp,
            "the_reference_has_noise_of_its_own": "its variance, about spp / reference_spp of a frame's, is inside the error and not inside the prediction",
            "calibration_reject_sigma_3": calibration[3.0], "calibration_reject_sigma_0": calibration[0.0],
            "false_rejections_reject_sigma_3": rejected,
            "mean_false_rejection_share": round(float(np.mean([r["share_of_hit_pixels_with_history_rejected"] for r in rejected])), 5)}


def moved_light(pt, width, height, frames, spp, reference_spp, light_step):
    from deform_scenes import rect_of

    host = load(pt, "cornell_mesh.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True, primitives=True)
    handles = {3.0: dev.temporal(width, height, cov=True), 0.0: dev.temporal(width, height, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=0.0))}
    rows, previous = [], None
    for k in range(frames):
        light = rect_of(host, LIGHT_RECT)
        light["corner"] = light["corner"] + np.array([light_step * (k - frames // 2), 0.0, 0.0], np.float32)
        dev.set_rects({LIGHT_RECT: light})
        s = host.settings_for(width=width, height=height, max_depth=8, seed=7000 + k)
        raw, cov, _ = dev.render_image_cov(s, spp)
        ref_settings = s.copy()
        ref_settings.seed = 9900 + k
        reference = dev.render_image(ref_settings, reference_spp)[0]
        outs = {sigma: t.step(s, raw, cov) for sigma, t in handles.items()}
        if previous is not None:
            changed = np.abs(lum(reference) - lum(previous)) > 0.05 * float(lum(reference).mean())
            rows.append({"frame": k, "changed_region_share": round(float(changed.mean()), 4),
                         **{"rmse_changed_sigma_%g" % sigma: rmse(out["rgb"], reference, changed) for sigma, out in outs.items()},
                         **{"rmse_unchanged_sigma_%g" % sigma: rmse(out["rgb"], reference, ~changed) for sigma, out in outs.items()},
                         "rmse_changed_raw": rmse(raw, reference, changed),
                         "share_of_hit_pixels_reset_by_the_test": round(float(((outs[3.0]["length"] == 1) & (outs[0.0]["length"] > 1)).mean()), 4)})
        previous = reference
    for t in handles.values():
        t.close()
    dev.close()
    mean = lambda key: round(float(np.mean([r[key] for r in rows if r[key] is not None])), 5)
    return {"scene": "scenes/cornell_mesh.scene", "width": width, "height": height, "frames": frames, "spp": spp, "reference_spp": reference_spp,
            "light_rectangle": LIGHT_RECT, "light_step_per_frame": light_step, "per_frame": rows,
            "mean": {key: mean(key) for key in ("changed_region_share", "rmse_changed_sigma_0", "rmse_changed_sigma_3", "rmse_unchanged_sigma_0",
                                                "rmse_unchanged_sigma_3", "rmse_changed_raw", "share_of_hit_pixels_reset_by_the_test")}}


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
    ap.add_argument("--light-step", type=float, default=12.0, help="units along x the light rectangle moves per frame (the box is 555 wide)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_cov_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch   # before the library is loaded: the two then share one HIP runtime

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    from scenes.gen_assets import ensure_assets

    if pt.device_count() < 1:
        raise SystemExit("tools/temporal_cov_cost.py needs a GPU")
    ensure_assets()
    seq = (args.seq_width, args.seq_height, args.frames, args.spp, args.reference_spp)
    report = {"timing": "device events around the accumulate group of a step on device-resident buffers, the plain and the covariance handle "
                        "stepped in turn, median of %d steps after %d warm-ups" % (args.rounds, args.warmups),
              "kernel": [kernel_cost(pt, torch, name, args.width, args.height, args.rounds, args.warmups)
                         for name in ("cornell_mesh.scene", "knot_glass.scene")],
              "turntable": turntable(pt, *seq), "static_pose": static_pose(pt, *seq), "moved_light": moved_light(pt, *seq, args.light_step)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
