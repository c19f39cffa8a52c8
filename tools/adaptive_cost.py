#!/usr/bin/env python3
"""What adaptive sampling (include/ptr_adaptive.h) costs and what it buys, in one job on one GPU: BASELINE configs[1] (Cornell box + OBJ
mesh, 1920x1080, depth 8, seed 1337), and the "buys" part again on the glass knot (configs[3] stand-in, depth 16).

  rounds   an adaptive frame with threshold 0 (nearly every pixel goes to maxSpp = 64; min 8, step 8) against ptr_render_bands_device at
           64 spp, whose code is the path every other entry point takes.  The two alternate in one process after a warm-up frame of each;
           wall time per frame.  The ratio is the price of eight ramp-ups and drains instead of one, plus the kernels between the rounds.
  update   k_adaptive_update between device events ([adaptive] lines of PTR_VERBOSE=launches).  Its least traffic is activeCount *
           roundSpp * 16 B of accumulators plus the state (3 + 3 + 6 floats read and written, n and e written) per active pixel; bytes
           over time against the HBM peak, beside k_resolve_cov of a 64-spp frame measured the same way in the same job.
  buys     three thresholds: the adaptive frame, and a uniform frame of ceil(mean count) spp (never fewer samples than the adaptive one);
           RMSE and relRMSE of both against a --reference-spp uniform render of seed 1338, the ratio of mean luminance to the reference
           for both (the bias of stopping on one's own samples), the histogram of counts; the same with the denoiser on the sample
           covariance applied to both.

  python tools/adaptive_cost.py [--out profiles/adaptive_cost.json]

Without --part the job runs its three parts (cost, cornell, knot) one after the other, each in a process of its own under a time limit
of its own, and stops at the first that fails; every part adds its figures to the report file.

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import math
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cov_cost import HBM_PEAK_BYTES_PER_S, launch_lines  # noqa: E402

LUMA = np.array([0.2126, 0.7152, 0.0722])


def errors(image, reference):
    a, r = image.astype(np.float64), reference.astype(np.float64)
    rmse = float(np.sqrt(np.mean((a - r) ** 2)))
    rel = float(np.sqrt(np.mean(((a - r) / (r + 1e-2)) ** 2)))      # the project's relRMSE (SURVEY.md section 8 d)
    return {"rmse": rmse, "rel_rmse": rel, "mean_luminance_ratio": float((a @ LUMA).mean() / (r @ LUMA).mean())}


def buys(pt, dev, s, thresholds, min_spp, step_spp, max_spp, reference_spp):
    other = s.copy()
    other.seed = 1338
    reference, _ = dev.render_image(other, reference_spp)
    albedo, normal = dev.render_aovs(s, 0)
    rows = []
    for thr in thresholds:
        p = pt.PtrAdaptiveParams(min_spp, max_spp, step_spp, thr)
        rgb, cov, count, stats, info = dev.render_adaptive(s, p)
        mean_count = float(count.mean())
        uniform_spp = max(2, int(math.ceil(mean_count)))
        u_rgb, u_cov, u_stats = dev.render_image_cov(s, uniform_spp)
        values, numbers = np.unique(count, return_counts=True)
        rows.append({
            "threshold": thr, "rounds": int(info.rounds), "mean_count": mean_count, "pixels_at_max": int(info.pixelsAtMax),
            "count_histogram": {str(int(v)): int(c) for v, c in zip(values, numbers)},
            "adaptive": dict(errors(rgb, reference), frame_ms=round(stats.totalSeconds * 1e3, 3)),
            "uniform": dict(errors(u_rgb, reference), spp=uniform_spp, frame_ms=round(u_stats.totalSeconds * 1e3, 3)),
            "adaptive_denoised": errors(pt.denoise(rgb, albedo, normal, cov=cov), reference),
            "uniform_denoised": errors(pt.denoise(u_rgb, albedo, normal, cov=u_cov), reference),
        })
    return {"reference_spp": reference_spp, "reference_seed": 1338, "min_spp": min_spp, "step_spp": step_spp, "max_spp": max_spp, "thresholds": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--thresholds", default="0.2,0.1,0.05")
    ap.add_argument("--part", choices=("cost", "cornell", "knot"), default=None, help="run this part only, in this process")
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds each part may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_cost.json"), help="the report file")
    args = ap.parse_args()
    if args.part is None:
        import subprocess

        if os.path.exists(args.out):
            os.remove(args.out)
        for part in ("cost", "cornell", "knot"):
            cmd = ["timeout", "-k", "10", str(args.part_timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--out", args.out,
                   "--width", str(args.width), "--height", str(args.height), "--rounds", str(args.rounds), "--reference-spp",
                   str(args.reference_spp), "--thresholds", args.thresholds]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("part %s ended with status %d: nothing more is started" % (part, rc), file=sys.stderr)
                sys.exit(rc)
        print(json.dumps(json.load(open(args.out))))
        return
    import torch

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    scenes = os.path.join(ROOT, "scenes")
    thresholds = [float(t) for t in args.thresholds.split(",")]
    report = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.part == "cost":
        report.update(cost(pt, torch, args, scenes))
    else:
        name, depth = ("cornell_mesh", 8) if args.part == "cornell" else ("knot_glass", 16)
        host = pt.HostScene.load(os.path.join(scenes, name + ".scene"), scenes)
        s = host.settings_for(width=args.width, height=args.height, max_depth=depth, seed=1337)
        dev = pt.DeviceScene(host.desc, 0, keepalive=host)
        report.setdefault("what_it_buys", {})[name] = dict(buys(pt, dev, s, thresholds, 8, 8, 64, args.reference_spp), max_depth=depth)
        dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


def cost(pt, torch, args, scenes):
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    rows = pt.band_count(args.height) * pt.BAND_ROWS
    pixels = args.width * args.height
    t_bands = torch.zeros((rows, args.width, 3), device="cuda")
    t_cov_bands = torch.zeros((rows, args.width, 6), device="cuda")
    t_rgb = torch.zeros((args.height, args.width, 3), device="cuda")
    t_cov = torch.zeros((args.height, args.width, 6), device="cuda")
    t_count = torch.zeros((args.height, args.width), device="cuda", dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    all_the_way = pt.PtrAdaptiveParams(8, 64, 8, 0.0)

    def wall(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0) * 1e3, out

    uniform = lambda: dev.render_device(s, 64, t_bands.data_ptr(), stream)
    adaptive = lambda: dev.render_adaptive_device(s, all_the_way, t_rgb.data_ptr(), t_cov.data_ptr(), t_count.data_ptr(), stream)
    uniform()
    adaptive()          # warm-up: buffers sized, kernels loaded
    ms = {"uniform_64": [], "adaptive_to_64": []}
    spans = {}
    for _ in range(args.rounds):
        t, st = wall(uniform)
        ms["uniform_64"].append(t)
        spans["uniform_64"] = st.as_dict()
        t, (st, info) = wall(adaptive)
        ms["adaptive_to_64"].append(t)
        spans["adaptive_to_64"] = st.as_dict()
    counts = t_count.cpu().numpy()
    at_max = float((counts == 64).mean())

    # the update kernel and its yardstick, between device events
    _, lines = launch_lines(adaptive)
    upd = [(int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4))) for m in
           (re.search(r"\[adaptive\] .*: (\d+) active x (\d+) spp; update ([0-9.]+) ms, select \+ compact ([0-9.]+) ms", l) for l in lines) if m]
    upd_rows = []
    for active, spp, update_ms, select_ms in upd:
        min_bytes = active * (spp * 16 + (12 * 4) * 2 + 8)
        upd_rows.append({"active": active, "spp": spp, "update_ms": update_ms, "select_compact_ms": select_ms, "min_bytes": min_bytes,
                         "fraction_of_hbm_peak": round(min_bytes / (update_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if update_ms > 0 else None})
    cov_call = lambda: dev.render_cov_device(s, 64, t_bands.data_ptr(), t_cov_bands.data_ptr(), stream)
    cov_call()
    cov_ms = []
    for _ in range(args.rounds):
        _, cl = launch_lines(cov_call)
        cov_ms.append(sum(float(m.group(1)) for m in (re.search(r"\[launch\] kind 4 .*\(([0-9.]+) ms\)", l) for l in cl) if m))
    cov_bytes = pixels * 64 * 16 + pixels * 24
    upd_runs = []
    for _ in range(args.rounds):
        _, ul = launch_lines(adaptive)
        upd_runs.append(sum(float(m.group(1)) for m in (re.search(r"update ([0-9.]+) ms", l) for l in ul) if m))
    upd_bytes = sum(r["min_bytes"] for r in upd_rows)

    report = {
        "scene": "scenes/cornell_mesh.scene", "resolution": [args.width, args.height], "max_depth": 8, "rounds": args.rounds,
        "cost_of_rounds": {
            "timing": "wall time per frame of alternating calls in one process after a warm-up of each; ms = best round",
            "params": {"min_spp": 8, "step_spp": 8, "max_spp": 64, "threshold": 0.0}, "pixels_at_64_fraction": at_max,
            "frame_ms": {k: {"ms_per_round": [round(x, 3) for x in v], "ms": round(min(v), 3)} for k, v in ms.items()},
            "adaptive_over_uniform": round(min(ms["adaptive_to_64"]) / min(ms["uniform_64"]), 4),
            "kernel_spans_last_round": spans,
        },
        "k_adaptive_update": {
            "timing": "device events around the launch (PTR_VERBOSE=launches), per round of one frame; totals over the frames of `rounds` runs",
            "per_round": upd_rows, "frame_total_ms_per_run": [round(x, 4) for x in upd_runs], "min_bytes_per_frame": upd_bytes,
            "fraction_of_hbm_peak": round(upd_bytes / (min(upd_runs) * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if upd_runs and min(upd_runs) > 0 else None,
            "k_resolve_cov_64spp": {"ms_per_run": [round(x, 4) for x in cov_ms], "min_bytes": cov_bytes,
                                    "fraction_of_hbm_peak": round(cov_bytes / (min(cov_ms) * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if min(cov_ms) > 0 else None},
            "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
        },
    }
    dev.close()
    return report


if __name__ == "__main__":
    main()
