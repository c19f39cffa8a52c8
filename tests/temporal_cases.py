"""Synthetic inputs of the temporal filter (include/ptr_temporal.h) for tests/test_temporal_host.py and tests/test_gpu_temporal.py: a
camera looking down -z at the plane z = -depth, one surface point per pixel centre, and records in which every pixel's point moved by a
given number of pixels.  With power-of-two image sides, pixel size and depth every projection here is exact in float32."""
import numpy as np

F = np.float32
MISS_BITS = np.array([0xFFFFFFFF], np.uint32).view(F)[0]


def camera(w, h, pixel=1.0 / 16.0, origin=(0.0, 0.0, 0.0)):
    """(o, ll, h, w) [4, 3]: pixel (x, y) of the w x h image is the square [x, x + 1] x [y, y + 1] * pixel of the plane one unit ahead."""
    o = np.array(origin, F)
    return np.array([o, o + np.array([-w * pixel / 2, -h * pixel / 2, -1.0], F), [w * pixel, 0, 0], [0, h * pixel, 0]], F)


def points(cam, w, h, fx, fy, depth=1.0):
    """World points the camera sees at pixel coordinates (fx, fy) [h, w] (row 0 on top) at `depth` along its axis."""
    o, ll, hh, ww = np.asarray(cam, F)
    u, v = (np.asarray(fx, F) / F(w))[..., None], (F(1) - np.asarray(fy, F) / F(h))[..., None]
    return (o + ((ll - o) + u * hh + v * ww) * F(depth)).astype(F)


def with_w(xyz, word):
    out = np.zeros(xyz.shape[:2] + (4,), F)
    out[..., :3] = xyz
    out[..., 3] = word
    return out


def bits(u):
    return np.asarray(u, np.uint32).view(F)


def plane_records(w, h, shift=(0.0, 0.0), cam=None, depth=1.0, ident=5):
    """(cur, prev) records of a plane facing the camera whose every point was `shift` pixels further right / down in the previous frame."""
    cam = camera(w, h) if cam is None else cam
    ys, xs = np.meshgrid(np.arange(h, dtype=F) + F(0.5), np.arange(w, dtype=F) + F(0.5), indexing="ij")
    x = points(cam, w, h, xs, ys, depth)
    x_prev = points(cam, w, h, xs + F(shift[0]), ys + F(shift[1]), depth)
    n = np.zeros((h, w, 3), F)
    n[..., 2] = 1
    word = np.full((h, w), ident, np.uint32).view(F)
    cur = [with_w(x, word), with_w(n, F(depth)), with_w(x_prev, bits(np.arange(w * h, dtype=np.uint32).reshape(h, w)))]
    prev = [with_w(x, word), with_w(n, F(depth))]
    return cur, prev


def history_of(rgb, length):
    return np.concatenate([np.asarray(rgb, F), np.broadcast_to(np.asarray(length, F), rgb.shape[:2])[..., None]], axis=2).astype(F)


def noisy_case(w, h, seed, motion, cam_cur, cam_prev):
    """A case with everything in it for the kernel-alone comparison: motion `motion` (pixels, may be fractional or leave the image) plus
    per-pixel jitter, miss pixels, NaN and inf colours, three ids in patches, tilted normals, points off the plane, histories of length
    0..7 with NaN colours among them."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=F) + F(0.5), np.arange(w, dtype=F) + F(0.5), indexing="ij")
    depth = (1.0 + 0.25 * xs / w + 0.003 * rng.random((h, w))).astype(F)[..., None]   # a slope, rough enough to pass and to miss the plane test
    jitter = ((rng.random((2, h, w)) - 0.5) * 0.6).astype(F)

    def cloud(cam, fx, fy):
        o = np.asarray(cam, F)[0]
        return (o + (points(cam, w, h, fx, fy) - o) * depth).astype(F)

    x = cloud(cam_cur, xs, ys)
    x_prev = cloud(cam_prev, xs + F(motion[0]) + jitter[0], ys + F(motion[1]) + jitter[1])
    x_tap = cloud(cam_prev, xs, ys)
    x_tap[..., 2] += np.where(rng.random((h, w)) < 0.15, 0.05, 0.0).astype(F)

    def normals():
        n = np.zeros((h, w, 3), F)
        n[..., 2] = 1
        tilt = rng.random((h, w)) < 0.2
        n[tilt] = np.array([0.6, 0.0, 0.8], F)
        return n

    ids = lambda: (rng.integers(0, 3, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.uint32) | np.uint32(1 << 31)).view(F)
    hit = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    hit[rng.random((h, w)) < 0.1] = 0xFFFFFFFF
    rgb = rng.random((h, w, 3)).astype(F)
    bad = rng.random((h, w))
    rgb[bad < 0.03, 1] = np.nan
    rgb[(bad > 0.03) & (bad < 0.05), 2] = np.inf
    cur = [with_w(x, ids()), with_w(normals(), depth[..., 0]), with_w(x_prev, hit.view(F))]
    prev = [with_w(x_tap, ids()), with_w(normals(), depth[..., 0])]
    hist_rgb = rng.random((h, w, 3)).astype(F)
    hist_rgb[rng.random((h, w)) < 0.05, 0] = np.nan
    history = history_of(hist_rgb, rng.integers(0, 8, (h, w)).astype(F))
    return rgb, cur, prev, history
