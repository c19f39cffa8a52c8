#!/usr/bin/env python3
"""What a resumable frame (include/ptr_frame.h) costs, in one job on one GPU: BASELINE configs[1] (Cornell box + OBJ mesh, 1920x1080,
depth 8, seed 1337).

  continued  a frame accumulated as 8 x 8 spp against ptr_render_bands_device at 64 spp, whose code is the path every other entry point
             takes.  The two alternate in one process after a warm-up of each; wall time per frame.  The ratio is the price of eight
             ramp-ups and drains instead of one, plus the update kernel between them.
  at_once    the same for one call of accumulate(64): what the frame's own state costs when nothing is continued.
  between    the kernels a refine adds between its rounds (class minimum + split, select on S + merge) between device events ([frame]
             lines of PTR_VERBOSE=launches), on a frame whose pixels hold different counts.  Their least traffic per round, over that
             time, against the HBM peak: the minimum and the split read the list and n (8 B per entry of L) and write a flag and S (1 B per
             entry, 4 B per entry of S); the merge reads the list, the flag and, for entries of S, n and nine values of e (5 B per entry,
             40 B per entry of S) and writes a flag and the next list (1 B + 4 B per kept entry).

  python tools/frame_cost.py [--out profiles/frame_cost.json]

Needs a GPU (no CPU fallback).  No figure here is a condition of any test; the report is printed as one JSON line either way.
"""
import argparse
import importlib
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cov_cost import HBM_PEAK_BYTES_PER_S, launch_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_cost.json"), help="the report file")
    args = ap.parse_args()
    import torch

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    rows = pt.band_count(args.height) * pt.BAND_ROWS
    t_bands = torch.zeros((rows, args.width, 3), device="cuda")
    t_rgb = torch.zeros((args.height, args.width, 3), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    frame = dev.frame(s)

    def wall(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    def continued():
        frame.reset()
        for _ in range(8):
            frame.accumulate(8, stream)
        frame.resolve_device(t_rgb.data_ptr(), stream=stream)

    def at_once():
        frame.reset()
        frame.accumulate(64, stream)
        frame.resolve_device(t_rgb.data_ptr(), stream=stream)

    uniform = lambda: dev.render_device(s, 64, t_bands.data_ptr(), stream)
    uniform()
    continued()
    at_once()          # warm-up: buffers sized, kernels loaded
    ms = {"uniform_64": [], "frame_8x8": [], "frame_1x64": []}
    for _ in range(args.rounds):
        ms["uniform_64"].append(wall(uniform))
        ms["frame_8x8"].append(wall(continued))
        ms["uniform_64"].append(wall(uniform))
        ms["frame_1x64"].append(wall(at_once))

    # the kernels between the rounds, on a frame with mixed counts: to 24 at a threshold that stops about half, then on at a lower one
    frame.reset()
    frame.refine(pt.PtrAdaptiveParams(8, 24, 8, 0.2), stream)
    _, lines = launch_lines(lambda: frame.refine(pt.PtrAdaptiveParams(8, 40, 8, 0.05), stream))
    between = []
    for line in lines:
        m = re.search(r"\[frame\] round (\d+): class (\d+), (\d+) of (\d+) active x (\d+) spp; minimum \+ split ([0-9.]+) ms, select \+ merge ([0-9.]+) ms", line)
        if not m:
            continue
        rnd, cls, in_s, active, spp = (int(m.group(i)) for i in range(1, 6))
        split_ms, merge_ms = float(m.group(6)), float(m.group(7))
        split_bytes = active * (8 + 1) + in_s * 4
        merge_bytes = active * (5 + 1 + 4) + in_s * 40
        between.append({"round": rnd, "class": cls, "in_class": in_s, "active": active, "spp": spp, "minimum_split_ms": split_ms,
                        "select_merge_ms": merge_ms, "minimum_split_min_bytes": split_bytes, "select_merge_min_bytes": merge_bytes,
                        "minimum_split_fraction_of_hbm_peak": round(split_bytes / (split_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 5) if split_ms > 0 else None,
                        "select_merge_fraction_of_hbm_peak": round(merge_bytes / (merge_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 5) if merge_ms > 0 else None})
    info = frame.info()
    best = {k: round(min(v), 3) for k, v in ms.items()}
    report = {
        "scene": "scenes/cornell_mesh.scene", "resolution": [args.width, args.height], "max_depth": 8, "rounds": args.rounds,
        "timing": "wall time per frame of alternating calls in one process after a warm-up of each; ms = best round",
        "frame_ms": {k: {"ms_per_round": [round(x, 3) for x in v], "ms": best[k]} for k, v in ms.items()},
        "continued_8x8_over_uniform": round(best["frame_8x8"] / best["uniform_64"], 4),
        "at_once_1x64_over_uniform": round(best["frame_1x64"] / best["uniform_64"], 4),
        "between_rounds": {
            "timing": "device events around the launches (PTR_VERBOSE=launches), per round of one refine on a frame with mixed counts "
                      "(minimum + split is the sum of the two spans; the host's read of the class minimum lies between them, in neither)",
            "counts_after": [int(info.minCount), int(info.maxCount)], "per_round": between, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
        },
    }
    frame.close()
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
