"""The temporal filter of include/ptr_temporal.h restated in numpy, written from that header's text and sharing no code with the product.

Everything is float32 and in the order the header prescribes, so the kernel's output is compared with array_equal.  Whole-image array
operations; a tap that does not count has weight exactly 0 (x + 0 = x, so the sums are those of the taps that count, in tap order).

    accumulate(rgb, cur, prev, history, cam_cur, cam_prev, ...) -> (out rgb, length, new history)     one step of the filter
    surface_point(rows, u, v) / sphere_point(row, row0, P, c)                                          X and Xprev of the records
"""
import numpy as np

F = np.float32
MISS = np.uint32(0xFFFFFFFF)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def project(cam, y, width, height):
    """Step 3: (fx, fy, valid) of the points y [..., 3] through cam = (o, ll, h, w), a [4, 3] float32 array."""
    o, ll, h, w = (np.asarray(cam, F).reshape(4, 3)[k] for k in range(4))
    d = y - o
    cn = cross(h, w)
    big_l = ll - o
    den = dot(d, cn)
    num = dot(big_l, cn)
    s = num / den
    valid = (s > 0) & np.isfinite(s)
    r = d * s[..., None] - big_l
    u = dot(r, h) / dot(h, h)
    v = dot(r, w) / dot(w, w)
    return u * F(width), (F(1) - v) * F(height), valid


def accumulate(rgb, cur, prev, history, cam_cur, cam_prev, max_history=32, normal_cos=0.9, plane_tolerance=0.01, has_history=True):
    """rgb [H, W, 3]; cur = (R0, R1, R2) and prev = (R0, R1) of [H, W, 4]; history [H, W, 4] -> (out [H, W, 3], length [H, W], history)."""
    rgb = np.asarray(rgb, F)
    h, w = rgb.shape[:2]
    r0, r1, r2 = (np.asarray(r, F).reshape(h, w, 4) for r in cur)
    p0, p1 = (np.asarray(r, F).reshape(h, w, 4) for r in prev)
    history = np.asarray(history, F).reshape(h, w, 4)
    with np.errstate(all="ignore"):
        miss = (r2[..., 3].view(np.uint32) == MISS) | ~np.isfinite(rgb).all(axis=2)
        out = rgb.copy()
        length = np.where(miss, F(0), F(1))
        if has_history:
            x_prev, n = r2[..., :3], r1[..., :3]
            fcx, fcy, ok_c = project(cam_cur, r0[..., :3], w, h)
            fpx, fpy, ok_p = project(cam_prev, x_prev, w, h)
            ys, xs = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
            sx, sy = xs + (fpx - fcx), ys + (fpy - fcy)
            ok = ~miss & ok_c & ok_p & np.isfinite(sx) & np.isfinite(sy)
            x0, y0 = np.floor(sx), np.floor(sy)
            ax, ay = sx - x0, sy - y0
            bx, by = (F(1) - ax, ax), (F(1) - ay, ay)
            to_camera = x_prev - np.asarray(cam_prev, F).reshape(4, 3)[0]
            bound = F(plane_tolerance) * np.sqrt(dot(to_camera, to_camera))
            big_b, sn, sc = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
            for k in range(4):
                b = bx[k & 1] * by[k >> 1]
                tx, ty = x0 + F(k & 1), y0 + F(k >> 1)
                inside = ok & (b > 0) & (tx >= 0) & (tx < F(w)) & (ty >= 0) & (ty < F(h))
                qx, qy = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
                hq, q0, q1 = history[qy, qx], p0[qy, qx], p1[qy, qx]
                nq = q1[..., :3]
                counts = inside & (hq[..., 3] >= 1) & np.isfinite(hq[..., :3]).all(axis=2) & \
                    (q0[..., 3].view(np.uint32) == r0[..., 3].view(np.uint32)) & (dot(nq, n) >= F(normal_cos)) & \
                    (np.abs(dot(x_prev - q0[..., :3], nq)) <= bound)
                b = np.where(counts, b, F(0))
                big_b = big_b + b
                sc = sc + b[..., None] * np.where(counts[..., None], hq[..., :3], F(0))
                sn = sn + b * np.where(counts, hq[..., 3], F(0))
            blend = big_b > 0
            hist = sc / big_b[..., None]
            grown = np.minimum(sn / big_b + F(1), F(max_history))
            a = F(1) / grown
            out = np.where(blend[..., None], hist + (rgb - hist) * a[..., None], rgb)
            length = np.where(blend, grown, length)
        out = out.astype(F)
        length = length.astype(F)
    return out, length, np.concatenate([out, length[..., None]], axis=2)


def surface_point(rows, u, v):
    """X of a triangle hit: rows [n, 3, 4] = (v0, v0 - v1, v2 - v0) in the xyz of each row, barycentrics u, v [n]."""
    rows = np.asarray(rows, F)
    u, v = np.asarray(u, F)[:, None], np.asarray(v, F)[:, None]
    return (rows[:, 0, :3] - u * rows[:, 1, :3]) + v * rows[:, 2, :3]


def sphere_point(row, row0, point):
    """X of a sphere hit: row [n, 4] = (c, r) the row to express the point on, row0 the row the ray hit, point = origin + t * direction."""
    row, row0, point = np.asarray(row, F), np.asarray(row0, F), np.asarray(point, F)
    return row[:, :3] + (point - row0[:, :3]) * (row[:, 3] / row0[:, 3])[:, None]
