"""numpy restatements of three rules include/ptr_appearance.h keeps to the bit (tests/test_appearance_host.py holds each against the
host probes): which rectangles are lights and in what order, the 2x2 mip rule, and Vose's alias method as the upload runs it."""
import numpy as np

f32 = np.float32
DIFFUSE_LIGHT = 3


def light_table(desc):
    """(lightIndexByRect [rects] int32, [(rectangle, emission rgb, two-sided)] per light in table order) of a description."""
    index = np.full(desc.rectCount, -1, np.int32)
    lights = []
    if desc.materialCount == 0:
        return index, lights
    for i in range(desc.rectCount):
        r = desc.rects[i]
        m = desc.materials[min(r.materialTwoSided[0], desc.materialCount - 1)]
        e = np.array(list(m.emission)[:3], f32)
        if int(m.typeEta[0]) != DIFFUSE_LIGHT or not (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > 0:
            continue
        index[i] = len(lights)
        lights.append((i, e, 1.0 if r.materialTwoSided[1] else 0.0))
    return index, lights


def mip_chain(level0):
    """Every level of the chain over level0 [h, w, 4] float32: sizes halve down to at least 1, at most 16 levels, a texel is
    ((a + b) + (c + d)) * 0.25 of the 2x2 block under it with the second tap clamped."""
    chain = [np.ascontiguousarray(level0, f32)]
    while (chain[-1].shape[0] > 1 or chain[-1].shape[1] > 1) and len(chain) < 16:
        src = chain[-1]
        h, w = src.shape[:2]
        nh, nw = max(h // 2, 1), max(w // 2, 1)
        y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
        x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
        a, b = src[y0][:, x0], src[y0][:, x1]
        c, d = src[y1][:, x0], src[y1][:, x1]
        chain.append((((a + b) + (c + d)) * f32(0.25)).astype(f32))
    return chain


def alias_table(prob):
    """(threshold float32, alias uint32) of the probabilities prob: work lists consumed from the back, an over-full entry moves to the
    under-full list once it drops below 1 - 1e-7, and what is left on either list gets threshold 1 and itself as alias."""
    n = len(prob)
    scaled = (np.asarray(prob, f32) * f32(n)).astype(f32)
    thr, alias = np.zeros(n, f32), np.zeros(n, np.uint32)
    under = [i for i in range(n) if scaled[i] < f32(1)]
    over = [i for i in range(n) if not scaled[i] < f32(1)]
    limit = f32(1) - f32(1e-7)
    while under and over:
        u = under.pop()
        o = over[-1]
        thr[u], alias[u] = min(max(scaled[u], f32(0)), f32(1)), o
        scaled[o] = f32(f32(scaled[o] + scaled[u]) - f32(1))
        if scaled[o] < limit:
            over.pop()
            under.append(o)
    for i in under + over:
        thr[i], alias[i] = f32(1), i
    return thr, alias


def env_tables(rgba):
    """The importance tables of a map [h, w, 4] by the upload's rule, from the alias loop above; the cell weights use numpy's float32 sine,
    so the caller compares the tables' alias structure and thresholds only where that sine agrees (the test says where)."""
    rgba = np.asarray(rgba, f32)
    h, w = rgba.shape[:2]
    d_theta, d_phi = f32(np.pi) / f32(h), f32(f32(2) * f32(np.pi)) / f32(w)
    cell = (np.maximum(np.sin((np.arange(h, dtype=f32) + f32(0.5)) * d_theta).astype(f32), f32(0)) * d_theta * d_phi).astype(f32)
    lum = ((f32(0.2126) * rgba[..., 0] + f32(0.7152) * rgba[..., 1]) + f32(0.0722) * rgba[..., 2]).astype(f32)
    weight = (np.maximum(lum, f32(0)) * cell[:, None]).astype(f32)
    row, total = np.zeros(h, f32), f32(0)
    for y in range(h):
        for x in range(w):
            row[y] = f32(row[y] + weight[y, x])
            total = f32(total + weight[y, x])
    return cell, weight, row, total
