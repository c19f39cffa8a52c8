#!/usr/bin/env python3
"""Generates tests/golden/vectors/cornell_32x32_d4_4spp_lumvar.json from the oracle (oracle/liboracle.so): what the per-pixel sample
covariance of include/ptr_stats.h has to add up to.

  python tests/golden/make_variance_golden.py            # rewrite the fixture
  python tests/golden/make_variance_golden.py --check    # regenerate in memory and compare with the committed file

S: the Cornell scene at 32x32, depth 4, 4 spp, rendered by the oracle with the seeds 1..256; per pixel the across-seed variance
(unbiased) of the image's luminance, summed over the pixels.  It is what sum over pixels of k^T C k estimates from ONE frame, with C the
covariance of the pixel mean and k the luminance weights - in expectation the two are equal, so their ratio over many seeds is 1.
half_difference: |S(seeds 1..128) - S(seeds 129..256)| / S, the fixture's own noise.
oracle_ratios: the same estimate made with the oracle alone, to show the test's band holds for an implementation known to be right:
six repetitions, each 128 groups of four 1-spp oracle renders (distinct seeds) taken as the four samples of a pixel; the mean over the
groups of sum_pixels k^T C k, divided by S.  tests/test_stats_host.py asserts that they lie in the band of tests/test_gpu_stats.py.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(HERE, "vectors", "cornell_32x32_d4_4spp_lumvar.json")

LUMA = np.array([0.2126, 0.7152, 0.0722])
WIDTH = HEIGHT = 32
DEPTH, SPP, SEEDS = 4, 4, 256
REPETITIONS, GROUPS, FIRST_SAMPLE_SEED = 6, 128, 100000


def generate():
    pt = importlib.import_module("metal-pathtracer-arm64_amd")
    import oracle_lib as ol
    from scenes.gen_assets import ensure_assets
    from stats_ref import two_pass64

    ensure_assets()      # the scene's mesh is a generated asset
    host = pt.HostScene.load(os.path.join(HERE, "cornell_small_mesh.scene"), os.path.join(ROOT, "scenes"))
    osc = ol.OracleScene(host)

    def render(seed, spp):
        s = host.settings_for(width=WIDTH, height=HEIGHT, max_depth=DEPTH, seed=seed)
        return osc.render(s, spp, threads=0)[0].astype(np.float64)

    lum = np.stack([render(seed, SPP) @ LUMA for seed in range(1, SEEDS + 1)])
    total = lambda a: float(a.var(axis=0, ddof=1).sum())
    s_all = total(lum)
    ratios = []
    seed = FIRST_SAMPLE_SEED
    for _ in range(REPETITIONS):
        sums = []
        for _ in range(GROUPS):
            samples = np.stack([render(seed + j, 1) for j in range(SPP)])
            seed += SPP
            c = two_pass64(samples)      # rr, gg, bb, rg, rb, gb
            k = LUMA
            quad = (k[0] * k[0] * c[..., 0] + k[1] * k[1] * c[..., 1] + k[2] * k[2] * c[..., 2]
                    + 2.0 * (k[0] * k[1] * c[..., 3] + k[0] * k[2] * c[..., 4] + k[1] * k[2] * c[..., 5]))
            sums.append(float(quad.sum()))
        ratios.append(float(np.mean(sums)) / s_all)
    return {"generator": "tests/golden/make_variance_golden.py", "scene": "cornell_small_mesh.scene", "width": WIDTH, "height": HEIGHT,
            "depth": DEPTH, "spp": SPP, "seeds": [1, SEEDS], "luma": LUMA.tolist(), "S": s_all,
            "half_difference": abs(total(lum[:SEEDS // 2]) - total(lum[SEEDS // 2:])) / s_all, "oracle_ratios": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = generate()
    if args.check:
        have = json.load(open(PATH))
        flat = lambda d: [d["S"], d["half_difference"]] + list(d["oracle_ratios"])
        same = len(flat(have)) == len(flat(out)) and np.allclose(flat(have), flat(out), rtol=1e-9, atol=0.0)
        print("differences:", "none" if same else (flat(have), flat(out)))
        sys.exit(0 if same else 1)
    json.dump(out, open(PATH, "w"), indent=1)
    print("wrote", PATH, "S = %.6g, half difference %.3f, oracle ratios %s" % (out["S"], out["half_difference"],
                                                                               ["%.3f" % r for r in out["oracle_ratios"]]))


if __name__ == "__main__":
    main()
