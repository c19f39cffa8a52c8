#!/usr/bin/env python3
"""What a resumable frame on several devices (include/ptr_multi_frame.h) saves and costs, in one job on whatever devices the machine
has: BASELINE configs[1] (Cornell box + OBJ mesh, 1920x1080, depth 8, seed 1337), min 4 / step 4, threshold 0.05.

  series    a 4 / 16 / 64-spp series - refine to maxSpp 4, then 16, then 64, a resolve after each - on ONE MultiFrame, whose scene is
            prepared and uploaded once at create, against the same three images from three one-shot ptr_render_multi_adaptive calls
            (the entry point as the parent commit has it), each of which prepares and uploads the scene again.  Wall time of every
            call from Python.  The resumed frame picks stopped pixels up again, so its sample totals are at or above the one-shot's
            at 16 and 64; both are reported.  The first step is checked to be bit-identical.
  rounds    per partition and refine: seconds in the call and of those waiting for the others (PtrMultiInfo); with more than one
            partition the two halves of the exchange between device events ([multi-frame] lines of PTR_VERBOSE=launches).
            With --ids 0,0 two partitions share one device: NOT a scaling figure.
  kernels   k_multi_state_pack / k_multi_state_unpack between device events on an export and an import of the 64-spp state: bytes
            moved (14 words read + 14 written per pixel) / time, against the 8 TB/s HBM peak of the MI355X.

  python tools/multi_frame_cost.py [--ids 0,0] [--out profiles/multi_frame_cost.json]

Every figure no run produced is the string "not measured".  Needs a GPU (no CPU fallback).  No figure here is a condition of any test.
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
from cov_cost import launch_lines  # noqa: E402

NOT_MEASURED = "not measured"
HBM_PEAK_BYTES_PER_S = 8.0e12
HALO = re.compile(r"\[multi-frame\] partition (\d+) round (\d+): class (\d+), (\d+) entries x (\d+) spp; halo (\d+) bytes each way; "
                  r"pack \+ copy ([0-9.]+) ms, copy \+ unpack ([0-9.]+) ms")
KERNEL = re.compile(r"\[multi-frame\] partition (\d+) (k_multi_state_(?:un)?pack): (\d+) bytes, ([0-9.]+) ms")
SERIES = (4, 16, 64)


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ids", default="", help="comma-separated device ids (repeats allowed); default: all visible devices")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_frame_cost.json"))
    args = ap.parse_args()

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    ids = [int(v) for v in args.ids.split(",")] if args.ids else None
    shared = ids is not None and len({i if i >= 0 else -(i + 1) for i in ids}) < len(ids)
    report = {"config": "cornell_mesh %dx%d depth 8 seed 1337, min 4 / step 4, threshold %g, series %s" % (args.width, args.height, args.threshold, list(SERIES)),
              "devices_visible": pt.device_count(), "device_ids": ids if ids is not None else "all visible",
              "series": NOT_MEASURED, "rounds": NOT_MEASURED, "kernels": NOT_MEASURED}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")

    if pt.device_count() < 1:
        save()
        print(json.dumps(report))
        return 0
    scenes = os.path.join(ROOT, "scenes")
    host = pt.HostScene.load(os.path.join(scenes, "cornell_mesh.scene"), scenes)
    s = host.settings_for(width=args.width, height=args.height, max_depth=8, seed=1337)
    params = [pt.PtrAdaptiveParams(4, n, 4, args.threshold) for n in SERIES]
    pt.render_multi_adaptive(host.desc, s, params[0], device_ids=ids)          # warm-up: code objects, the BVH builder's threads

    # ---- the series on one frame, and its rounds
    def frame_series():
        rows = []
        frame, create_s = timed(lambda: pt.multi_frame(host.desc, s, device_ids=ids))
        for p in params:
            (stats, info), refine_s = timed(lambda: frame.refine(p))
            multi = frame.multi_info()
            image, resolve_s = timed(lambda: frame.resolve())
            rows.append({"max_spp": int(p.maxSpp), "refine_s": refine_s, "resolve_s": resolve_s, "samples_of_the_call": int(info.totalSamples),
                         "samples_in_the_frame": int(frame.info().totalSamples), "adaptive_rounds": int(info.rounds),
                         "partitions": [{"samples": a, "call_s": b, "wait_s": c} for a, b, c in multi.per_part()], "image": image})
        return frame, create_s, rows

    frame, create_s, rows = frame_series()                # timed without PTR_VERBOSE: its device events and prints cost time
    parts = int(frame.multi_info().parts)
    halo = []
    if parts > 1:                                          # a second frame, verbose, for the exchange between device events
        def verbose_refine():
            other = pt.multi_frame(host.desc, s, device_ids=ids)
            other.refine(params[1])
            other.close()
        _, lines = launch_lines(verbose_refine)
        halo = [m.groups() for m in (HALO.search(l) for l in lines) if m]
    one_shot = []
    for p in params:
        out, call_s = timed(lambda: pt.render_multi_adaptive(host.desc, s, p, device_ids=ids))
        one_shot.append({"max_spp": int(p.maxSpp), "whole_call_s": call_s, "of_which_prepare_and_upload_s": out["stats"].uploadSeconds,
                         "samples": int(out["info"].totalSamples), "image": (out["rgb"], out["cov"], out["count"])})
    import numpy as np
    same_first = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(rows[0]["image"], one_shot[0]["image"]))
    for row in rows + one_shot:
        del row["image"]
    frame_total = create_s + sum(r["refine_s"] + r["resolve_s"] for r in rows)
    report["series"] = {"multi_frame": {"create_s (scene prepared once, uploaded to every device once)": create_s, "steps": rows, "total_s": frame_total},
                        "one_shot_calls": {"steps": one_shot, "total_s": sum(r["whole_call_s"] for r in one_shot)},
                        "first_step_bit_identical": bool(same_first), "partitions": parts}
    report["rounds"] = {"exchange (a second frame refined to 16 under PTR_VERBOSE=launches)": [{"partition": int(a), "round": int(b), "class": int(c), "entries": int(d), "spp": int(e), "halo_bytes_each_way": int(f),
                                      "pack_and_copy_ms": float(g), "copy_and_unpack_ms": float(h)} for a, b, c, d, e, f, g, h in halo] or
                        "one partition: no exchange",
                        "note": "partitions that share a device: not a scaling figure" if shared else ""}
    save()

    # ---- the two checkpoint kernels
    state = frame.export_state()                           # warm-up of both: the first launch loads the code object
    frame.import_state(state)
    found = []
    for _ in range(5):
        state, lines_out = launch_lines(frame.export_state)
        _, lines_in = launch_lines(lambda: frame.import_state(state))
        found += lines_out + lines_in
    kernels = {}
    for m in (KERNEL.search(l) for l in found):
        if not m:
            continue
        part, name, nbytes, ms = int(m.group(1)), m.group(2), int(m.group(3)), float(m.group(4))
        rate = nbytes / (ms * 1e-3) if ms > 0 else 0.0
        kernels.setdefault(name, []).append({"partition": part, "bytes": nbytes, "ms": ms, "bytes_per_s": rate,
                                             "fraction_of_8_TB_per_s": rate / HBM_PEAK_BYTES_PER_S})
    report["kernels"] = kernels or NOT_MEASURED
    frame.close()
    save()
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
