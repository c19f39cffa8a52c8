#!/usr/bin/env python3
"""What the denoiser (include/ptr_post.h) costs and gains at full size: BASELINE configs[1] (Cornell box + OBJ mesh, 1920x1080, depth 8,
seed 1337) rendered at 16 spp, its first-hit feature buffers, and the filter with its defaults on them.

Every kernel (prepare, each a-trous pass, finish) is timed between device events: the mean of 20 runs after 5 warm-up runs, for both
kernel variants (PTR_DENOISE_TILED=0: every tap through the caches; =1: staged in LDS wherever a tiled kernel exists), the two
alternating over --rounds rounds in one process.  Per kernel the report gives the bytes the pass has to move at least (each input read
once, each output written once) over its time as a fraction of the HBM peak, and which variant the library's default picks.  The RMSE
against a --reference-spp render before and after the filter is tests/test_gpu_denoise.py::test_it_denoises at full size.

  python tools/denoise_bench.py [--out profiles/denoise_1080p.json]

Needs a GPU (no CPU fallback); the report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X HBM3E, specified peak
# bytes per pixel a kernel has to move: prepare reads rgb, albedo, normal and writes colour, guide, slope; a pass reads colour, guide,
# slope and writes colour; finish reads rgb, albedo, guide, colour and writes rgb
BYTES_PER_PIXEL = {"prepare": 12 + 16 + 16 + 16 + 16 + 4, "pass": 16 + 16 + 4 + 16, "finish": 12 + 16 + 16 + 16 + 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=512)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    image, stats = dev.render_image(s, args.spp)
    albedo, normal = dev.render_aovs(s, 0)
    other = s.copy()
    other.seed = 4242
    reference, _ = dev.render_image(other, args.reference_spp)
    dev.close()

    params = pt.PtrDenoiseParams.defaults()
    names = ["prepare"] + ["pass_step_%d" % (1 << i) for i in range(params.iterations)] + ["finish"]
    kinds = ["prepare"] + ["pass"] * params.iterations + ["finish"]
    pixels = args.width * args.height
    t_rgb, t_albedo, t_normal = (torch.from_numpy(a).cuda() for a in (image, albedo, normal))
    t_out = torch.zeros_like(t_rgb)
    variants = {"simple": "0", "tiled": "1"}
    times = {v: [] for v in variants}
    images = {}
    for _ in range(args.rounds):
        for variant, knob in variants.items():
            os.environ["PTR_DENOISE_TILED"] = knob
            ms, tiled = pt.denoise_timed(t_rgb.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), args.width, args.height, t_out.data_ptr(),
                                         params, runs=args.runs, warmup=args.warmup)
            times[variant].append(ms)
            images[variant] = t_out.cpu().numpy()
    del os.environ["PTR_DENOISE_TILED"]
    _, default_tiled = pt.denoise_timed(t_rgb.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), args.width, args.height, t_out.data_ptr(),
                                        params, runs=1, warmup=0)
    denoised = pt.denoise(image, albedo, normal, params)

    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - reference.astype(np.float64)) ** 2)))
    kernels = {}
    for k, (name, kind) in enumerate(zip(names, kinds)):
        row = {"bytes": BYTES_PER_PIXEL[kind] * pixels, "default_is_tiled": bool(default_tiled[k])}
        for variant in variants:
            per_round = [r[k] for r in times[variant]]
            best = min(per_round)
            row[variant] = {"ms_per_round": [round(v, 4) for v in per_round], "ms": round(best, 4),
                            "fraction_of_hbm_peak": round(row["bytes"] / (best * 1e-3) / HBM_PEAK_BYTES_PER_S, 4)}
        row["has_tiled_kernel"] = kind == "prepare" or (kind == "pass" and (1 << (k - 1)) <= 4)
        kernels[name] = row
    report = {
        "scene": "scenes/cornell_mesh.scene", "resolution": [args.width, args.height], "max_depth": 8, "spp": args.spp,
        "runs": args.runs, "warmup": args.warmup, "rounds": args.rounds, "timing": "device events around every kernel, mean of the runs; ms = best round",
        "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "iterations": params.iterations,
        "kernels": kernels,
        "total_ms": {v: round(sum(kernels[n][v]["ms"] for n in names), 4) for v in variants},
        "total_ms_default": round(sum(kernels[n]["tiled" if kernels[n]["default_is_tiled"] else "simple"]["ms"] for n in names), 4),
        "render_ms": round(stats.totalSeconds * 1e3, 3),
        "variants_bit_identical": bool(np.array_equal(images["simple"], images["tiled"]) and np.array_equal(images["simple"], denoised)),
        "rmse": {"reference_spp": args.reference_spp, "reference_seed": 4242, "before": rmse(image), "after": rmse(denoised),
                 "ratio": rmse(denoised) / rmse(image)},
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
