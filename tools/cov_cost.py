#!/usr/bin/env python3
"""What the per-pixel sample covariance (include/ptr_stats.h) costs and what the denoiser gains from it, in one job: BASELINE configs[1]
(Cornell box + OBJ mesh, 1920x1080, depth 8, seed 1337).

  cost   the frame at --spp (256) with and without the covariance output, alternating in one process after a warm-up frame of each.  The
         yardstick is the frame WITHOUT it: that is the path every other entry point takes.  k_resolve_cov itself is timed between device
         events (the [launch] kind 4 lines of PTR_VERBOSE=launches, read back from the library's stderr); the bytes it has to move at least
         - every per-sample accumulator once (16 B), the running mean of a frame of several passes (16 B per pixel, read and written between
         passes) and the output (24 B per pixel) - over that time is given as a fraction of the HBM peak.
  gain   at --denoise-spp (16): the RMSE of the raw image, of the denoiser on its 7x7 spatial variance and of the denoiser on the sample
         covariance, against a --reference-spp (512) render of another seed.

  python tools/cov_cost.py [--out profiles/cov_cost.json]

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X HBM3E, specified peak


def launch_lines(call):
    """Runs call() with PTR_VERBOSE=launches and the process's stderr (the library prints with fprintf) in a file: (result, its lines)."""
    sys.stderr.flush()
    saved = os.dup(2)
    before = os.environ.get("PTR_VERBOSE")
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        os.environ["PTR_VERBOSE"] = "launches"
        try:
            result = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            if before is None:
                del os.environ["PTR_VERBOSE"]
            else:
                os.environ["PTR_VERBOSE"] = before
        f.seek(0)
        return result, f.read().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--denoise-spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    rows = pt.band_count(args.height) * pt.BAND_ROWS
    pixels = args.width * args.height
    t_rgb = torch.zeros((rows, args.width, 3), device="cuda")
    t_cov = torch.zeros((rows, args.width, 6), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    plain = lambda: dev.render_device(s, args.spp, t_rgb.data_ptr(), stream).totalSeconds * 1e3
    with_cov = lambda: dev.render_cov_device(s, args.spp, t_rgb.data_ptr(), t_cov.data_ptr(), stream).totalSeconds * 1e3
    plain()
    with_cov()          # warm-up: buffers sized, kernels loaded
    ms = {"without_cov": [], "with_cov": []}
    for _ in range(args.rounds):
        ms["without_cov"].append(plain())
        image_plain = t_rgb.cpu().numpy()
        ms["with_cov"].append(with_cov())
        same_image = bool(np.array_equal(t_rgb.cpu().numpy(), image_plain))
    _, lines = launch_lines(with_cov)
    kernel_ms = [float(m.group(1)) for m in (re.search(r"\[launch\] kind 4 .*\(([0-9.]+) ms\)", l) for l in lines) if m]
    passes = len(kernel_ms)
    # every accumulator once; the mean is written by every pass but the last and read by every pass but the first; the output is written by
    # every pass and read back by every pass but the first
    min_bytes = pixels * args.spp * 16 + max(passes - 1, 0) * pixels * (16 + 16 + 24) + max(passes, 1) * pixels * 24
    kernel_total = sum(kernel_ms)

    # the denoiser on the two variances
    img, cov, _ = dev.render_image_cov(s, args.denoise_spp)
    albedo, normal = dev.render_aovs(s, 0)
    other = s.copy()
    other.seed = 4242
    reference, _ = dev.render_image(other, args.reference_spp)
    dev.close()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - reference.astype(np.float64)) ** 2)))
    spatial, spatial_ms = pt.denoise(img, albedo, normal, return_ms=True)
    sample, sample_ms = pt.denoise(img, albedo, normal, return_ms=True, cov=cov)

    best = {k: min(v) for k, v in ms.items()}
    report = {
        "scene": "scenes/cornell_mesh.scene", "resolution": [args.width, args.height], "max_depth": 8, "spp": args.spp, "rounds": args.rounds,
        "timing": "PtrRenderStats.totalSeconds of alternating frames in one process after a warm-up frame of each; ms = best round",
        "frame_ms": {k: {"ms_per_round": [round(x, 3) for x in v], "ms": round(best[k], 3)} for k, v in ms.items()},
        "cov_cost_fraction_of_frame": round(best["with_cov"] / best["without_cov"] - 1.0, 5),
        "image_unchanged_by_cov": same_image,
        "k_resolve_cov": {"timing": "device events around the launch (PTR_VERBOSE=launches, kind 4), one frame", "passes": passes,
                          "ms_per_pass": [round(x, 4) for x in kernel_ms], "ms": round(kernel_total, 4), "min_bytes": min_bytes,
                          "fraction_of_hbm_peak": round(min_bytes / (kernel_total * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if kernel_total > 0 else None,
                          "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S},
        "denoise": {"spp": args.denoise_spp, "reference_spp": args.reference_spp, "reference_seed": 4242,
                    "rmse": {"raw": rmse(img), "spatial_variance": rmse(spatial), "sample_variance": rmse(sample)},
                    "kernel_ms": {"spatial_variance": round(spatial_ms, 4), "sample_variance": round(sample_ms, 4)}},
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
