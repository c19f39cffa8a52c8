"""The temporal filter that carries covariance (include/ptr_temporal_cov.h) restated in numpy, written from that header's text and from
ptr_temporal.h's, and sharing no code with the product.

Everything is float32 and in the order the headers prescribe, so the kernel's output is compared with array_equal.  Whole-image array
operations, as in temporal_ref, whose project and dot these are; a tap that does not count has weight exactly 0 and its values are taken
as 0 (x + 0 * 0 = x), so every sum is that of the taps that count, in tap order.  temporal_ref.accumulate keeps its taps to itself, so
counting_taps below walks them once more by step 5 of ptr_temporal.h; that the walk is temporal_ref's is held by
tests/test_temporal_cov_host.py: with reject_sigma 0 colour, length and colour history equal temporal_ref.accumulate's bit for bit.

    accumulate_cov(rgb, cov, cur, prev, history, cov_history, cam_cur, cam_prev, ...)
        -> (out rgb, length, new history, out cov, new cov history)                                    one step of the filter
    lum(x) / lumvar(c6)                                                                                 the two projections on luminance
"""
import numpy as np

import temporal_ref as ref

F = np.float32
K = (F(0.2126), F(0.7152), F(0.0722))
AT = ((0, 3, 4), (3, 1, 5), (4, 5, 2))   # where C_cd is among (rr, gg, bb, rg, rb, gb)


def lum(x):
    return (K[0] * x[..., 0] + K[1] * x[..., 1]) + K[2] * x[..., 2]


def lumvar(c6):
    v = np.zeros(c6.shape[:-1], F)
    for c in range(3):
        for d in range(3):
            v = v + (K[c] * K[d]) * c6[..., AT[c][d]]
    return np.where(np.isfinite(v) & (v > 0), v, F(0)).astype(F)


def counting_taps(ok, r0, r1, r2, p0, p1, history, cam_cur, cam_prev, normal_cos, plane_tolerance):
    """Steps 3-5 of ptr_temporal.h for the pixels `ok` (neither a miss nor without a finite colour): four (b, qy, qx), b the weight of tap
    k where it counts and 0 elsewhere, (qy, qx) the tap's pixel ((0, 0) where b is 0)."""
    h, w = ok.shape
    x_prev, n = r2[..., :3], r1[..., :3]
    fcx, fcy, ok_c = ref.project(cam_cur, r0[..., :3], w, h)
    fpx, fpy, ok_p = ref.project(cam_prev, x_prev, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    sx, sy = xs + (fpx - fcx), ys + (fpy - fcy)
    ok = ok & ok_c & ok_p & np.isfinite(sx) & np.isfinite(sy)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    bx, by = (F(1) - ax, ax), (F(1) - ay, ay)
    to_camera = x_prev - np.asarray(cam_prev, F).reshape(4, 3)[0]
    bound = F(plane_tolerance) * np.sqrt(ref.dot(to_camera, to_camera))
    taps = []
    for k in range(4):
        b = bx[k & 1] * by[k >> 1]
        tx, ty = x0 + F(k & 1), y0 + F(k >> 1)
        inside = ok & (b > 0) & (tx >= 0) & (tx < F(w)) & (ty >= 0) & (ty < F(h))
        qx, qy = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
        hq, q0, q1 = history[qy, qx], p0[qy, qx], p1[qy, qx]
        nq = q1[..., :3]
        counts = inside & (hq[..., 3] >= 1) & np.isfinite(hq[..., :3]).all(axis=2) & \
            (q0[..., 3].view(np.uint32) == r0[..., 3].view(np.uint32)) & (ref.dot(nq, n) >= F(normal_cos)) & \
            (np.abs(ref.dot(x_prev - q0[..., :3], nq)) <= bound)
        taps.append((np.where(counts, b, F(0)).astype(F), np.where(counts, qy, 0), np.where(counts, qx, 0)))
    return taps


def accumulate_cov(rgb, cov, cur, prev, history, cov_history, cam_cur, cam_prev, max_history=32, normal_cos=0.9, plane_tolerance=0.01,
                   reject_sigma=3.0, has_history=True):
    """rgb [H, W, 3]; cov [H, W, 6]; cur = (R0, R1, R2) and prev = (R0, R1) of [H, W, 4]; history [H, W, 4]; cov_history [H, W, 6]
    -> (out [H, W, 3], length [H, W], history [H, W, 4], out_cov [H, W, 6], cov history [H, W, 6])."""
    rgb = np.asarray(rgb, F)
    h, w = rgb.shape[:2]
    cov = np.asarray(cov, F).reshape(h, w, 6)
    r0, r1, r2 = (np.asarray(r, F).reshape(h, w, 4) for r in cur)
    p0, p1 = (np.asarray(r, F).reshape(h, w, 4) for r in prev)
    history = np.asarray(history, F).reshape(h, w, 4)
    cov_history = np.asarray(cov_history, F).reshape(h, w, 6)
    rs = F(reject_sigma)
    with np.errstate(all="ignore"):
        cc = np.where(np.isfinite(cov), cov, F(0)).astype(F)
        miss = (r2[..., 3].view(np.uint32) == ref.MISS) | ~np.isfinite(rgb).all(axis=2)
        out = rgb.copy()
        length = np.where(miss, F(0), F(1))
        out_cov = np.where(miss[..., None], F(0), cc)     # step 1; step 2 and every reset
        if has_history:
            big_b, sn = np.zeros((h, w), F), np.zeros((h, w), F)
            sc, sv = np.zeros((h, w, 3), F), np.zeros((h, w, 6), F)
            for b, qy, qx in counting_taps(~miss, r0, r1, r2, p0, p1, history, cam_cur, cam_prev, normal_cos, plane_tolerance):
                counts = (b > 0)[..., None]
                hq, vq = history[qy, qx], cov_history[qy, qx]
                big_b = big_b + b
                sc = sc + b[..., None] * np.where(counts, hq[..., :3], F(0))
                sn = sn + b * np.where(counts[..., 0], hq[..., 3], F(0))
                sv = sv + b[..., None] * np.where(counts, vq, F(0))
            found = big_b > 0
            hist = sc / big_b[..., None]
            big_h = sv / big_b[..., None]
            d = lum(rgb) - lum(hist)
            v = lumvar(cc) + lumvar(big_h.astype(F))
            rejected = found & (rs > 0) & (d * d > (rs * rs) * v)
            blend = found & ~rejected
            grown = np.minimum(sn / big_b + F(1), F(max_history))
            a = F(1) / grown
            k = F(1) - a
            out = np.where(blend[..., None], hist + (rgb - hist) * a[..., None], rgb)
            length = np.where(blend, grown, length)
            blended = (k * k)[..., None] * big_h + (a * a)[..., None] * cc
            blended = np.where(np.isfinite(blended), blended, cc)
            out_cov = np.where(blend[..., None], blended, out_cov)
        out, length, out_cov = out.astype(F), length.astype(F), out_cov.astype(F)
    return out, length, np.concatenate([out, length[..., None]], axis=2), out_cov, out_cov.copy()
