"""The denoiser on a measured variance (include/ptr_stats.h, ptr_denoise_cov) restated in numpy, written from the text of that header
and of include/ptr_post.h and sharing no code with the product.  It has a prepare of its own - the variance v_p comes from the covariance
of the pixel means - and borrows the helpers of tests/denoise_ref.py (image shifts, luminance, depth slope, guide weights) for the parts
the two filters have in common.  Parametrised by dtype like denoise_ref: float64 is the reference, float32 the yardstick for rounding.
"""
import numpy as np

from denoise_ref import B3, _axis_slope, _guide_weights, _luminance, _shifted

LUMA = (0.2126, 0.7152, 0.0722)
# C_cd of the symmetric matrix -> entry of the six stored (rr, gg, bb, rg, rb, gb)
ENTRY = ((0, 3, 4), (3, 1, 5), (4, 5, 2))


def pixel_variance(cov, a, T):
    """v_q of the header for every pixel: sum over c, d of (g_c g_d) C_cd with g = k / a; 0 unless finite and positive."""
    cov = np.asarray(cov, dtype=np.float32).astype(T)
    g = [T(LUMA[c]) / a[..., c] for c in range(3)]
    v = np.zeros(cov.shape[:2], dtype=T)
    with np.errstate(all="ignore"):
        for c in range(3):
            for d in range(3):
                v = v + (g[c] * g[d]) * cov[..., ENTRY[c][d]]
        return np.where(np.isfinite(v) & (v > 0), v, T(0))


def prefilter(v, hit, T):
    """v_p of the header: the 3x3 weighted mean of v over the in-image hit pixels (0 at miss pixels)."""
    sum_w, sum_wv = np.zeros_like(v), np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = T((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25))
            present = _shifted(hit, dy, dx, False)
            sum_w = sum_w + np.where(present, w, T(0))
            sum_wv = sum_wv + np.where(present, w * _shifted(v, dy, dx, T(0)), T(0))
    with np.errstate(all="ignore"):
        return np.where(hit, sum_wv / np.where(hit, sum_w, T(1)), T(0))


def denoise_cov_ref_all(rgb, albedo, normal, cov, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0, flags=1,
                        dtype=np.float64, return_variance=False):
    """The filter's output after 1, 2, ... `iterations` a-trous passes (a list of [H, W, 3] arrays of `dtype`).  return_variance: the
    prepared v_p instead."""
    T = np.dtype(dtype).type
    sl, sn, sz = T(np.float32(sigma_luminance)), T(np.float32(sigma_normal)), T(np.float32(sigma_depth))
    rgb_in = np.asarray(rgb, dtype=np.float32)
    albedo = np.asarray(albedo, dtype=np.float32)
    normal = np.asarray(normal, dtype=np.float32)
    hit = (albedo[..., 3] > 0.5) & (normal[..., 3] > 0) & np.isfinite(rgb_in).all(axis=2)
    with np.errstate(all="ignore"):
        # prepare: decode, guide and slope as include/ptr_post.h has them
        rgbT = rgb_in.astype(dtype)
        a = np.maximum(albedo[..., :3].astype(dtype), T(1e-3)) if flags & 1 else np.ones_like(rgbT)
        c = np.where(hit[..., None], rgbT / a, T(0))
        m = T(2) * normal[..., :3].astype(dtype) - T(1)
        length = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        n = np.where(length[..., None] > 0, m / np.where(length > 0, length, T(1))[..., None], T(0))
        z = np.where(hit, normal[..., 3].astype(dtype), T(-1))
        slope = np.maximum(_axis_slope(z, _shifted(z, 0, -1, T(-1)), _shifted(z, 0, 1, T(-1)), T),
                           _axis_slope(z, _shifted(z, -1, 0, T(-1)), _shifted(z, 1, 0, T(-1)), T))
        z_term = T(1e-3) * z
        # ... and the variance of include/ptr_stats.h
        v = prefilter(pixel_variance(cov, a, T), hit, T)
        if return_variance:
            return v

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


def denoise_cov_ref(rgb, albedo, normal, cov, **kw):
    return denoise_cov_ref_all(rgb, albedo, normal, cov, **kw)[-1]
