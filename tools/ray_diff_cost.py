#!/usr/bin/env python3
"""Cost of the first-hit ray differentials (PTR_METAL_RAY_DIFF) on a textured scene at full size: tests/golden/textured.scene (a glTF
with base-colour, ORM, normal and emissive maps) at 1920x1080, depth 6, 64 spp.  metalSemantics 127 vs 127|256 and 32 vs 32|256; the
values of one round are rendered one after the other and the rounds repeat, so the two of each pair alternate.

  python tools/ray_diff_cost.py [--rounds 3] [--spp 64] [--semantics 127,383,32,288] [--out report.json]

PTR_HIP_LIBRARY=<other libptr_hip.so> measures another build the same way (an A/B against the parent commit).  The report is printed
as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--semantics", default="127,383,32,288", help="comma-separated metalSemantics values, measured in this order")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    golden = os.path.join(ROOT, "tests", "golden")
    host = pt.HostScene.load(os.path.join(golden, "textured.scene"), golden)
    s = host.settings_for(width=args.width, height=args.height, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    values = [int(v) for v in args.semantics.split(",")]
    report = {"scene": "tests/golden/textured.scene", "resolution": [s.width, s.height], "max_depth": s.maxDepth, "spp": args.spp,
              "library": os.environ.get("PTR_HIP_LIBRARY", "in-tree"), "rounds": args.rounds}
    for sem in values:   # warm-up of every instantiation
        w = s.copy()
        w.metalSemantics = sem
        dev.render_image(w, 4)
    samples = s.width * s.height * args.spp
    rates = {sem: [] for sem in values}
    for _ in range(args.rounds):
        for sem in values:
            r = s.copy()
            r.metalSemantics = sem
            _, st = dev.render_image(r, args.spp)
            rates[sem].append(round(samples / st.totalSeconds / 1e6, 1))
    median = {sem: sorted(v)[len(v) // 2] for sem, v in rates.items()}
    report["msamples_per_s"] = {str(k): v for k, v in rates.items()}
    report["median"] = {str(k): v for k, v in median.items()}
    report["change_with_bit"] = {"%d_vs_%d" % (sem, sem | 256): round(median[sem | 256] / median[sem] - 1.0, 4)
                                 for sem in values if not sem & 256 and (sem | 256) in median}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
