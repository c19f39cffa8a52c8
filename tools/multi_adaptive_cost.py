#!/usr/bin/env python3
"""What the multi-device protocol of include/ptr_multi.h costs, in one job on whatever devices the machine has: BASELINE configs[1]
(Cornell box + OBJ mesh, 1920x1080, depth 8, seed 1337), min 8 / step 8 / max 64, thresholds 0 and 0.05.

  protocol  (a) the price of the protocol on one device: ptr_render_multi_adaptive with one partition against ptr_render_adaptive, the
            parent's code path, alternating in one process after a warm-up of each; mean of --frames frames, --rounds rounds, with the
            spread.  Compared like with like: the wall time of either whole call from Python, both returning rgb, cov and count, the
            multi call's less the preparation and upload of the scene it reports (ptr_render_adaptive works on an uploaded scene).
            Beside it partRenderSeconds[0] (the rounds, finish and hand-over alone: NOT comparable with a whole call) and, from one
            verbose call, where the rest of the multi call goes: the first device's buffers, the partition's state (allocated and zeroed
            per call), interleave + download, the release of the scene.
  exchange  (b) ids [0, 0]: two partitions on one device.  Halo bytes per round and partition, pack + copy and copy + unpack between
            device events ([multi] lines of PTR_VERBOSE=launches), wait seconds per partition.  NOT a scaling figure.
  scaling   (c) only where more than one device is visible: N = 1, 2, 4, 8 devices with per-partition samples, render and wait seconds.

  python tools/multi_adaptive_cost.py [--out profiles/multi_adaptive_cost.json]

Every figure no run produced is the string "not measured".  Needs a GPU (no CPU fallback).  No figure here is a condition of any test.
"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cov_cost import launch_lines  # noqa: E402

NOT_MEASURED = "not measured"
PART = re.compile(r"\[ptr\]   device (\d+): \d+ bands, \d+ samples, upload ([0-9.]+) s, state ([0-9.]+) s, render ([0-9.]+) s, of which waiting ([0-9.]+) s")
OUTSIDE = re.compile(r"outside the partitions' threads: first-device buffers ([0-9.]+) s, interleave \+ download ([0-9.]+) s, release of the scenes ([0-9.]+) s")
WHOLE = re.compile(r"\[ptr\] \d+ device\(s\): scene preparation ([0-9.]+) s, .* whole call ([0-9.]+) s")
HALO = re.compile(r"\[multi\] partition (\d+) round (\d+): halo (\d+) bytes each way; pack \+ copy ([0-9.]+) ms, copy \+ unpack ([0-9.]+) ms")


def spread(values):
    return {"mean": statistics.fmean(values), "min": min(values), "max": max(values), "n": len(values)}


def stderr_lines(call):
    """call() with the process's stderr (the library prints with fprintf) in a file: (result, its lines)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        try:
            result = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return result, f.read().splitlines()


def breakdown(lines):
    """Where one verbose multi call spent its time, in seconds, from the library's own report."""
    text = "\n".join(lines)
    whole, part, outside = WHOLE.search(text), PART.search(text), OUTSIDE.search(text)
    if not (whole and part and outside):
        return NOT_MEASURED
    row = {"whole_call_in_library": float(whole.group(2)), "scene_preparation": float(whole.group(1)), "scene_upload": float(part.group(2)),
           "state_allocated_and_zeroed": float(part.group(3)), "rounds_finish_hand_over": float(part.group(4)),
           "first_device_buffers": float(outside.group(1)), "interleave_and_download": float(outside.group(2)),
           "release_of_the_scene": float(outside.group(3))}
    row["unaccounted"] = row["whole_call_in_library"] - sum(v for k, v in row.items() if k != "whole_call_in_library")
    return row


def parts_of(out):
    return [{"samples": a, "render_s": b, "wait_s": c} for a, b, c in out["multi"].per_part()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-spp", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_adaptive_cost.json"))
    args = ap.parse_args()

    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    report = {"config": "cornell_mesh %dx%d depth 8 seed 1337, min 8 / step 8 / max %d" % (args.width, args.height, args.max_spp),
              "devices_visible": pt.device_count(), "protocol": NOT_MEASURED, "exchange": NOT_MEASURED, "scaling": NOT_MEASURED,
              "exchange_between_two_devices": NOT_MEASURED}

    def save():
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
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)

    # (a) one partition against the single-device entry point
    protocol = {}
    for thr in (0.0, 0.05):
        p = pt.PtrAdaptiveParams(8, args.max_spp, 8, thr)
        dev.render_adaptive(s, p, want_cov=True, want_count=True)                    # warm-up of each
        pt.render_multi_adaptive(host.desc, s, p, device_ids=[0])
        rounds = []
        for _ in range(args.rounds):
            single, multi, call, upload = [], [], [], []
            for _ in range(args.frames):
                t0 = time.perf_counter()
                dev.render_adaptive(s, p)
                single.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                out = pt.render_multi_adaptive(host.desc, s, p, device_ids=[0])
                call.append(time.perf_counter() - t0)
                multi.append(out["multi"].partRenderSeconds[0])
                upload.append(out["stats"].uploadSeconds)
            rest = [c - u for c, u in zip(call, upload)]
            rounds.append({"single_whole_call_s": spread(single), "multi_whole_call_s": spread(call), "multi_prepare_and_upload_s": spread(upload),
                           "multi_call_less_upload_s": spread(rest), "ratio_of_means_call_less_upload_to_single": statistics.fmean(rest) / statistics.fmean(single),
                           "multi_rounds_finish_hand_over_s (not comparable with a whole call)": spread(multi)})
        _, lines = stderr_lines(lambda: pt.render_multi_adaptive(host.desc, s, p, n_devices=1, verbose=True))
        protocol["threshold %g" % thr] = {"rounds": rounds, "samples": int(out["info"].totalSamples), "adaptive_rounds": int(out["info"].rounds),
                                          "one_verbose_multi_call_s": breakdown(lines)}
        report["protocol"] = protocol
        save()

    # (b) two partitions on one device: the exchange between device events
    exchange = {}
    for thr in (0.0, 0.05):
        p = pt.PtrAdaptiveParams(8, args.max_spp, 8, thr)
        out, lines = launch_lines(lambda: pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, 0]))
        rows = [HALO.search(l) for l in lines]
        rows = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))) for m in rows if m]
        exchange["threshold %g" % thr] = {
            "note": "two partitions share one device: not a scaling figure",
            "halo_bytes_per_round_each_way": sorted({r[2] for r in rows}),
            "pack_and_copy_ms": spread([r[3] for r in rows]) if rows else NOT_MEASURED,
            "copy_and_unpack_ms": spread([r[4] for r in rows]) if rows else NOT_MEASURED,
            "adaptive_rounds": int(out["info"].rounds), "partitions": parts_of(out)}
        report["exchange"] = exchange
        save()

    # (c) real devices
    if pt.device_count() > 1:
        scaling = {}
        for thr in (0.0, 0.05):
            p = pt.PtrAdaptiveParams(8, args.max_spp, 8, thr)
            row = {}
            for n in (1, 2, 4, 8):
                if n > pt.device_count():
                    row["N=%d" % n] = NOT_MEASURED
                    continue
                pt.render_multi_adaptive(host.desc, s, p, n_devices=n)      # warm-up
                out = pt.render_multi_adaptive(host.desc, s, p, n_devices=n)
                row["N=%d" % n] = {"render_s": out["stats"].totalSeconds, "staged_parts": int(out["multi"].stagedParts), "partitions": parts_of(out)}
            scaling["threshold %g" % thr] = row
        report["scaling"] = scaling
        report["exchange_between_two_devices"] = "ran (see scaling)"
    save()
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
