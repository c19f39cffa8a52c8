#!/usr/bin/env python3
"""Cost of the prefiltered environment lookups (PTR_METAL_ENV_LOD) on BASELINE config 3 (helmet_env.scene at full size: 1920x1080,
depth 8, 256 spp): metalSemantics 127 vs 255 and 32 vs 32|128, the two of each pair alternated, plus the time to build the mip chain of
the 2048x1024 map (first render with the bit on a fresh upload).

  python tools/env_lod_cost.py [--rounds 3] [--out report.json]   (the report is printed as one JSON line either way)
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    from scenes.gen_assets import ensure_assets

    ensure_assets()
    host = pt.HostScene.load(os.path.join(ROOT, "scenes", "helmet_env.scene"), os.path.join(ROOT, "scenes"))
    s = host.settings_for(width=1920, height=1080, max_depth=8, seed=1337)
    report = {"scene": "helmet_env.scene", "resolution": [s.width, s.height], "max_depth": s.maxDepth, "spp": args.spp, "pairs": {}}

    # the chain: PTR_VERBOSE=build prints its milliseconds; timed here around the first render with the bit (1 spp, small frame)
    os.environ["PTR_VERBOSE"] = "build"
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    small = s.copy()
    small.width, small.height, small.metalSemantics = 64, 64, 255
    t0 = time.perf_counter()
    dev.render_image(small, 1)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev.render_image(small, 1)
    second = time.perf_counter() - t0
    del os.environ["PTR_VERBOSE"]
    report["first_render_with_bit_s"] = round(first, 4)
    report["second_render_with_bit_s"] = round(second, 4)

    samples = s.width * s.height * args.spp
    for off, on in ((127, 255), (32, 32 | 128)):
        rates = {off: [], on: []}
        for sem in (off, on):   # warm-up of both instantiations
            w = s.copy()
            w.metalSemantics = sem
            dev.render_image(w, 4)
        for _ in range(args.rounds):
            for sem in (off, on):
                r = s.copy()
                r.metalSemantics = sem
                _, st = dev.render_image(r, args.spp)
                rates[sem].append(round(samples / st.totalSeconds / 1e6, 1))
        med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        report["pairs"]["%d_vs_%d" % (off, on)] = {"msamples_per_s": {str(k): v for k, v in rates.items()},
                                                    "median": {str(k): v for k, v in med.items()},
                                                    "change": round(med[on] / med[off] - 1.0, 4)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
