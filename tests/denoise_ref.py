"""The denoiser of include/ptr_post.h restated in numpy, written from that header's text and sharing no code with the product.

One function, parametrised by dtype: float64 is the reference; float32 does the same operations in the same order as the header (and so
the kernels) prescribes and is the yardstick for what float32 rounding alone does to the result.  Whole-image array operations: a tap
(dx, dy) is the image shifted by it, a skipped tap a weight of exactly 0 (x + 0 = x, so the sums are those of the taps that count).
"""
import numpy as np

B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def _shifted(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx] where that is in the image, `fill` elsewhere."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def _luminance(c, T):
    return (T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1]) + T(0.0722) * c[..., 2]


def _axis_slope(z, zm, zp, T):
    m, p = zm > 0, zp > 0
    return np.where(m & p, np.abs(zp - zm) / T(2), np.where(p, np.abs(zp - z), np.where(m, np.abs(zm - z), T(0))))


def _guide_weights(n, z, nq, zq, slope, step_dist, z_term, sigma_n, sigma_z):
    d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
    wn = np.power(np.maximum(0, d), sigma_n)
    wz = np.exp(-np.abs(z - zq) / (sigma_z * (slope * step_dist + z_term)))
    return wn, wz


def denoise_ref_all(rgb, albedo, normal, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0, flags=1, dtype=np.float64):
    """The filter's output after 1, 2, ... `iterations` a-trous passes (a list of [H, W, 3] arrays of `dtype`): entry i - 1 is what the
    filter returns for iterations = i, since prepare and the earlier passes do not depend on how many follow."""
    T = np.dtype(dtype).type
    sl, sn, sz = T(np.float32(sigma_luminance)), T(np.float32(sigma_normal)), T(np.float32(sigma_depth))
    rgb_in = np.asarray(rgb, dtype=np.float32)
    albedo = np.asarray(albedo, dtype=np.float32)
    normal = np.asarray(normal, dtype=np.float32)
    hit = (albedo[..., 3] > 0.5) & (normal[..., 3] > 0) & np.isfinite(rgb_in).all(axis=2)
    with np.errstate(all="ignore"):
        rgbT = rgb_in.astype(dtype)
        a = np.maximum(albedo[..., :3].astype(dtype), T(1e-3)) if flags & 1 else np.ones_like(rgbT)
        c = np.where(hit[..., None], rgbT / a, T(0))
        lum = _luminance(c, T)
        m = T(2) * normal[..., :3].astype(dtype) - T(1)
        length = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        n = np.where(length[..., None] > 0, m / np.where(length > 0, length, T(1))[..., None], T(0))
        z = np.where(hit, normal[..., 3].astype(dtype), T(-1))
        slope = np.maximum(_axis_slope(z, _shifted(z, 0, -1, T(-1)), _shifted(z, 0, 1, T(-1)), T),
                           _axis_slope(z, _shifted(z, -1, 0, T(-1)), _shifted(z, 1, 0, T(-1)), T))
        z_term = T(1e-3) * z

        # variance: two passes over the 7x7 window, weights k = wn * wz at step 1, the centre 1
        def window():
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    zq = _shifted(z, dy, dx, T(-1))
                    if dx == 0 and dy == 0:
                        k = np.ones_like(z)
                    else:
                        wn, wz = _guide_weights(n, z, _shifted(n, dy, dx, T(0)), zq, slope, np.sqrt(T(dx * dx + dy * dy)), z_term, sn, sz)
                        k = wn * wz
                    yield np.where(zq > 0, k, T(0)), np.where(zq > 0, _shifted(lum, dy, dx, T(0)), T(0))

        sum_k, sum_kl = np.zeros_like(z), np.zeros_like(z)
        for k, lq in window():
            sum_k = sum_k + k
            sum_kl = sum_kl + k * lq
        mean = sum_kl / sum_k
        sum_kd = np.zeros_like(z)
        for k, lq in window():
            d = lq - mean
            sum_kd = sum_kd + k * (d * d)
        v = np.where(hit, sum_kd / sum_k, T(0))

        outs = []
        for i in range(iterations):
            s = 1 << i
            lp = _luminance(c, T)
            den_l = sl * np.sqrt(v) + T(1e-6)
            sw = np.zeros_like(z)
            sc = np.zeros_like(c)
            sv = np.zeros_like(z)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    zq = _shifted(z, s * dy, s * dx, T(-1))
                    cq = _shifted(c, s * dy, s * dx, T(0))
                    h = T(B3[dx + 2]) * T(B3[dy + 2])
                    if dx == 0 and dy == 0:
                        w = np.full_like(z, h)
                    else:
                        wn, wz = _guide_weights(n, z, _shifted(n, s * dy, s * dx, T(0)), zq, slope, T(s) * np.sqrt(T(dx * dx + dy * dy)),
                                                z_term, sn, sz)
                        wl = np.exp(-np.abs(lp - _luminance(cq, T)) / den_l)
                        w = ((h * wn) * wz) * wl
                    w = np.where(zq > 0, w, T(0))
                    sw = sw + w
                    sc = sc + w[..., None] * cq
                    sv = sv + (w * w) * _shifted(v, s * dy, s * dx, T(0))
            c = np.where(hit[..., None], sc / sw[..., None], T(0))
            v = np.where(hit, sv / (sw * sw), T(0))
            outs.append(np.where(hit[..., None], c * a, rgbT))
    return outs


def denoise_ref(rgb, albedo, normal, **kw):
    return denoise_ref_all(rgb, albedo, normal, **kw)[-1]
