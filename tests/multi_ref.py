"""The multi-device adaptive frame of include/ptr_multi.h restated in numpy on top of tests/adaptive_ref.py, written from that header's
text and sharing no code with the product: P partitions of 8-row bands in lock-step rounds, each with an image-order error array of its
own that knows the other partitions' rows only through the halo.

halo = "true":  the protocol of the header.
halo = "none":  nothing is exchanged: rows of other partitions count as e = 0.
halo = "stale": the neighbour rows are exchanged after round 0 only and frozen there.
The two wrong variants exist to show that an input discriminates (tests/test_multi_host.py)."""
from types import SimpleNamespace

import numpy as np

import adaptive_ref

BAND = 8
F = np.float32


def band_count(height):
    return (height + BAND - 1) // BAND


def partition_pixels(width, height, part, parts):
    """The first list of partition `part`: its bands top to bottom, each in 8x8 blocks left to right, each block row-major."""
    out = []
    for b in range(part, band_count(height), parts):
        y0, y1 = b * BAND, min(b * BAND + BAND, height)
        for tx in range(0, width, 8):
            for y in range(y0, y1):
                for x in range(tx, min(tx + 8, width)):
                    out.append(y * width + x)
    return np.array(out, dtype=np.uint32)


def multi_ref(samples, p, parts, halo="true"):
    """samples [maxSpp, H, W, 3].  Returns rgb, cov, count, rounds, active_after (summed over the partitions), part_samples."""
    samples = np.asarray(samples, dtype=F)
    height, width = samples.shape[1:3]
    pixels = height * width
    flat = samples.reshape(samples.shape[0], pixels, 3)
    bands = band_count(height)
    states = [adaptive_ref.zero_state(pixels) for _ in range(parts)]
    active = [partition_pixels(width, height, q, parts) for q in range(parts)]
    owner = (np.arange(pixels) // width // BAND) % parts
    exchange = np.zeros((height, width), F)                       # the published rows, by image row
    out = SimpleNamespace(rounds=0, active_after=[], part_samples=[0] * parts)
    n = 0
    while sum(a.size for a in active) > 0 and n < p.maxSpp:
        spp = p.minSpp if n == 0 else min(p.stepSpp, p.maxSpp - n)
        for q in range(parts):                                    # update, then publish the edge rows of the own bands
            if active[q].size == 0:
                continue
            a = active[q]
            st, _, _ = adaptive_ref.round_ref(width, height, p, n, flat[n:n + spp][:, a], a, states[q], last=False)
            st["e"][a] = adaptive_ref.pixel_error(st["mean"][a], st["m"][a], n + spp)
            states[q] = st
            out.part_samples[q] += int(a.size) * spp
            e2 = st["e"].reshape(height, width)
            for b in range(q, bands, parts):
                exchange[b * BAND] = e2[b * BAND]
                last_row = min(b * BAND + BAND, height) - 1
                exchange[last_row] = e2[last_row]
        n += spp
        for q in range(parts):                                    # read the neighbours' rows, select, compact
            if active[q].size == 0:
                continue
            a = active[q]
            st = states[q]
            if parts > 1 and (halo == "true" or (halo == "stale" and out.rounds == 0)):
                e2 = st["e"].reshape(height, width)
                for b in range(q, bands, parts):
                    if b > 0:
                        e2[b * BAND - 1] = exchange[b * BAND - 1]
                    if b * BAND + BAND < height:
                        e2[b * BAND + BAND] = exchange[b * BAND + BAND]
            big = adaptive_ref.dilate(st["e"], width, height)
            keep = (st["n"][a] < p.maxSpp) & (big[a] > p.threshold)
            active[q] = a[keep]
        out.active_after.append(int(sum(a.size for a in active)))
        out.rounds += 1
    count = np.zeros(pixels, np.uint32)
    total = np.zeros((pixels, 3), F)
    m = np.zeros((pixels, 6), F)
    for q in range(parts):
        mine = owner == q
        count[mine], total[mine], m[mine] = states[q]["n"][mine], states[q]["sum"][mine], states[q]["m"][mine]
    with np.errstate(all="ignore"):
        out.rgb = (total / count.astype(F)[:, None]).reshape(height, width, 3)
        out.cov = (m / (count.astype(F) * (count - 1).astype(F))[:, None]).reshape(height, width, 6)
    out.count = count.reshape(height, width)
    return out


def median_threshold(samples, min_spp, step_spp):
    """The median of the first round's dilated error (how the tests place the threshold so that about half the pixels go on)."""
    first = adaptive_ref.adaptive_ref(samples[:min_spp], adaptive_ref.params(min_spp, min_spp, step_spp, 0.0))
    return float(np.median(first.E[0]))
