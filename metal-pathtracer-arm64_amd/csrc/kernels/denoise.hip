// The edge-avoiding a-trous wavelet denoiser on the first-hit feature buffers: prepare, one a-trous pass, finish.
// The filter is spelled out in include/ptr_post.h; this file follows that text line by line (float32, unfused: the Makefile compiles it
// with -ffp-contract=off, in the order written), and so does the numpy restatement the tests compare it with (tests/denoise_ref.py).
//
// Layout: colour rgb | variance as one float4 per pixel and the guide (unit normal | depth, depth <= 0 = miss pixel) as another, so a tap
// is two 16-byte loads; the depth slope g_p is read once per pixel from a float buffer of its own.  Colour ping-pongs between two buffers.
// One thread per pixel, 16x16 workgroups (four waves; a wave covers four rows of 16 pixels, 256 contiguous bytes per row and load).
//
// Two variants of prepare and of the passes at steps 1, 2 and 4, which differ only in where a tap comes from:
//   simple  every tap is read through the caches (prepare decodes each of its 49 taps from the raw inputs);
//   tiled   the block first stages its pixels plus the halo the taps reach, (16 + 4 s)^2 * 32 B <= 32 KB, in LDS (prepare decodes each
//           pixel of its 22x22 tile once).
// Both run the same per-pixel function (preparePixel / atrousPixel) on a fetch functor, so their images are the same bits.
#include <hip/hip_runtime.h>

#include "denoise.h"

namespace ptrk {

namespace {

constexpr int kTile = 16;        // workgroup side
constexpr int kVarRadius = 3;    // 7x7 variance window
constexpr int kTapRadius = 2;    // 5x5 a-trous taps

struct DenoiseConsts {
    float sigmaL, sigmaN, sigmaZ;
    uint32_t demodulate;
};

DenoiseConsts constsOf(const PtrDenoiseParams& p) {
    return DenoiseConsts{p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth, p.flags & PTR_DENOISE_DEMODULATE};
}

// what prepare knows of a pixel: colour = demodulated rgb | luminance, guide = unit normal | depth (<= 0: miss pixel)
struct Pixel {
    float4 colour, guide;
};

__device__ inline float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ inline float4 missGuide() { return make_float4(0.0f, 0.0f, 0.0f, -1.0f); }

__device__ inline float3 albedoDivisor(const float4& albedo, uint32_t demodulate) {
    if (!demodulate) return make_float3(1.0f, 1.0f, 1.0f);
    return make_float3(fmaxf(albedo.x, 1e-3f), fmaxf(albedo.y, 1e-3f), fmaxf(albedo.z, 1e-3f));
}

__device__ inline Pixel decodePixel(const float* rgb, const float4* albedo, const float4* normal, size_t i, uint32_t demodulate) {
    float r = rgb[i * 3 + 0], g = rgb[i * 3 + 1], b = rgb[i * 3 + 2];
    const float4 a = albedo[i], nz = normal[i];
    Pixel px;
    const bool hit = a.w > 0.5f && nz.w > 0.0f && __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b);
    if (!hit) {
        px.colour = make_float4(r, g, b, 0.0f);
        px.guide = missGuide();
        return px;
    }
    if (demodulate) {
        const float3 d = albedoDivisor(a, demodulate);
        r = r / d.x;
        g = g / d.y;
        b = b / d.z;
    }
    const float mx = 2.0f * nz.x - 1.0f, my = 2.0f * nz.y - 1.0f, mz = 2.0f * nz.z - 1.0f;
    const float len = sqrtf((mx * mx + my * my) + mz * mz);
    px.colour = make_float4(r, g, b, luminance(r, g, b));
    px.guide = len > 0.0f ? make_float4(mx / len, my / len, mz / len, nz.w) : make_float4(0.0f, 0.0f, 0.0f, nz.w);
    return px;
}

// wn and wz of a tap (dx, dy) at step s: stepDist = s * |(dx, dy)|, zTerm = 1e-3 * z_p
__device__ inline float normalWeight(const float4& gp, const float4& gq, float sigmaN) {
    const float d = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
    return powf(fmaxf(0.0f, d), sigmaN);
}

__device__ inline float depthWeight(const float4& gp, const float4& gq, float slope, float stepDist, float zTerm, float sigmaZ) {
    return expf(-fabsf(gp.w - gq.w) / (sigmaZ * (slope * stepDist + zTerm)));
}

__device__ inline float tapDistance(int dx, int dy) { return sqrtf(static_cast<float>(dx * dx + dy * dy)); }

// the depth slope along one axis: zMinus / zPlus are the neighbours' depths, <= 0 where the neighbour is out of the image or a miss
__device__ inline float axisSlope(float z, float zMinus, float zPlus) {
    const bool m = zMinus > 0.0f, p = zPlus > 0.0f;
    if (m && p) return fabsf(zPlus - zMinus) / 2.0f;
    if (p) return fabsf(zPlus - z);
    if (m) return fabsf(zMinus - z);
    return 0.0f;
}

// Prepare for the pixel (x, y) of the image.  fetch(qx, qy) -> Pixel of an in-image pixel.
template <typename Fetch>
__device__ inline void preparePixel(int x, int y, int width, int height, const DenoiseConsts& k, const DenoiseBuffers& buf, Fetch fetch) {
    const Pixel p = fetch(x, y);
    const size_t i = static_cast<size_t>(y) * width + x;
    buf.guide[i] = p.guide;
    if (!(p.guide.w > 0.0f)) return;   // a miss pixel: its colour and slope are never read
    auto depthAt = [&](int qx, int qy) { return (qx < 0 || qy < 0 || qx >= width || qy >= height) ? -1.0f : fetch(qx, qy).guide.w; };
    const float z = p.guide.w;
    const float slope = fmaxf(axisSlope(z, depthAt(x - 1, y), depthAt(x + 1, y)), axisSlope(z, depthAt(x, y - 1), depthAt(x, y + 1)));
    const float zTerm = 1e-3f * z;
    auto weightOf = [&](int dx, int dy, const Pixel& q) {
        if (dx == 0 && dy == 0) return 1.0f;
        return normalWeight(p.guide, q.guide, k.sigmaN) * depthWeight(p.guide, q.guide, slope, tapDistance(dx, dy), zTerm, k.sigmaZ);
    };
    float sumK = 0.0f, sumKl = 0.0f;
    for (int dy = -kVarRadius; dy <= kVarRadius; ++dy) {
        for (int dx = -kVarRadius; dx <= kVarRadius; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            const Pixel q = fetch(qx, qy);
            if (!(q.guide.w > 0.0f)) continue;
            const float kq = weightOf(dx, dy, q);
            sumK += kq;
            sumKl += kq * q.colour.w;
        }
    }
    const float mean = sumKl / sumK;
    float sumKd = 0.0f;
    for (int dy = -kVarRadius; dy <= kVarRadius; ++dy) {
        for (int dx = -kVarRadius; dx <= kVarRadius; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            const Pixel q = fetch(qx, qy);
            if (!(q.guide.w > 0.0f)) continue;
            const float d = q.colour.w - mean;
            sumKd += weightOf(dx, dy, q) * (d * d);
        }
    }
    buf.colour[0][i] = make_float4(p.colour.x, p.colour.y, p.colour.z, sumKd / sumK);
    buf.slope[i] = slope;
}

// ---- prepare on a measured variance (include/ptr_stats.h): v_p from the covariance of the pixel mean instead of the 7x7 window

// v_q of a hit pixel q: the variance of its demodulated luminance, sum over c, d of (g_c g_d) C_cd with g = k / albedo divisor
__device__ inline float luminanceVariance(const float* cov, size_t q, const float3& a) {
    const float g[3] = {0.2126f / a.x, 0.7152f / a.y, 0.0722f / a.z};
    const float* c = cov + q * 6u;   // rr, gg, bb, rg, rb, gb
    const float C[3][3] = {{c[0], c[3], c[4]}, {c[3], c[1], c[5]}, {c[4], c[5], c[2]}};
    float v = 0.0f;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) v += (g[i] * g[j]) * C[i][j];
    }
    return (__builtin_isfinite(v) && v > 0.0f) ? v : 0.0f;
}

// Prepare for the pixel (x, y) with v_p = the 3x3 prefilter of v_q.  Guide and depth slope as preparePixel writes them.
template <typename Fetch>
__device__ inline void preparePixelCov(int x, int y, int width, int height, const DenoiseConsts& k, const DenoiseBuffers& buf, const float4* albedo,
                                       const float* cov, Fetch fetch) {
    const Pixel p = fetch(x, y);
    const size_t i = static_cast<size_t>(y) * width + x;
    buf.guide[i] = p.guide;
    if (!(p.guide.w > 0.0f)) return;   // a miss pixel: its colour and slope are never read
    auto depthAt = [&](int qx, int qy) { return (qx < 0 || qy < 0 || qx >= width || qy >= height) ? -1.0f : fetch(qx, qy).guide.w; };
    const float z = p.guide.w;
    const float slope = fmaxf(axisSlope(z, depthAt(x - 1, y), depthAt(x + 1, y)), axisSlope(z, depthAt(x, y - 1), depthAt(x, y + 1)));
    float sumW = 0.0f, sumWv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            if (!(fetch(qx, qy).guide.w > 0.0f)) continue;
            const size_t q = static_cast<size_t>(qy) * width + qx;
            const float w = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);   // 1/4, 1/8, 1/16
            sumW += w;
            sumWv += w * luminanceVariance(cov, q, albedoDivisor(albedo[q], k.demodulate));
        }
    }
    buf.colour[0][i] = make_float4(p.colour.x, p.colour.y, p.colour.z, sumWv / sumW);
    buf.slope[i] = slope;
}

__device__ inline float b3(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// One a-trous pass at step s for the pixel (x, y).  fetch(qx, qy, colour, guide) reads an in-image pixel's colour | variance and guide.
template <typename Fetch>
__device__ inline void atrousPixel(int x, int y, int width, int height, int s, const DenoiseConsts& k, const float* slopes, float4* dst,
                                   Fetch fetch) {
    float4 cp, gp;
    fetch(x, y, cp, gp);
    if (!(gp.w > 0.0f)) return;   // a miss pixel: never read by a pass, copied from the input by finish
    const size_t i = static_cast<size_t>(y) * width + x;
    const float slope = slopes[i];
    const float lp = luminance(cp.x, cp.y, cp.z);
    const float denL = k.sigmaL * sqrtf(cp.w) + 1e-6f;
    const float zTerm = 1e-3f * gp.w;
    const float fs = static_cast<float>(s);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -kTapRadius; dy <= kTapRadius; ++dy) {
        for (int dx = -kTapRadius; dx <= kTapRadius; ++dx) {
            const int qx = x + s * dx, qy = y + s * dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            float4 cq, gq;
            fetch(qx, qy, cq, gq);
            if (!(gq.w > 0.0f)) continue;
            const float h = b3(dx) * b3(dy);
            float w = h;
            if (dx != 0 || dy != 0) {
                const float wn = normalWeight(gp, gq, k.sigmaN);
                const float wz = depthWeight(gp, gq, slope, fs * tapDistance(dx, dy), zTerm, k.sigmaZ);
                const float wl = expf(-fabsf(lp - luminance(cq.x, cq.y, cq.z)) / denL);
                w = ((h * wn) * wz) * wl;
            }
            sw += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
            sv += (w * w) * cq.w;
        }
    }
    dst[i] = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// ---- simple variant: taps through the caches

__global__ void __launch_bounds__(kTile* kTile) k_denoise_prepare(const float* rgb, const float4* albedo, const float4* normal, int width, int height,
                                                                   DenoiseConsts k, DenoiseBuffers buf) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    preparePixel(x, y, width, height, k, buf,
                 [&](int qx, int qy) { return decodePixel(rgb, albedo, normal, static_cast<size_t>(qy) * width + qx, k.demodulate); });
}

__global__ void __launch_bounds__(kTile* kTile) k_denoise_prepare_cov(const float* rgb, const float4* albedo, const float4* normal, const float* cov,
                                                                       int width, int height, DenoiseConsts k, DenoiseBuffers buf) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    preparePixelCov(x, y, width, height, k, buf, albedo, cov,
                    [&](int qx, int qy) { return decodePixel(rgb, albedo, normal, static_cast<size_t>(qy) * width + qx, k.demodulate); });
}

__global__ void __launch_bounds__(kTile* kTile) k_denoise_atrous(int width, int height, int step, DenoiseConsts k, const float4* src,
                                                                  const float4* guide, const float* slopes, float4* dst) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    atrousPixel(x, y, width, height, step, k, slopes, dst, [&](int qx, int qy, float4& c, float4& g) {
        const size_t q = static_cast<size_t>(qy) * width + qx;
        c = src[q];
        g = guide[q];
    });
}

// ---- tiled variant: the block's pixels and their halo staged in LDS.  Out-of-image tile entries are never fetched (the per-pixel
// functions test the image bounds first); they are still written, as miss pixels, so no LDS word is left undefined.

__global__ void __launch_bounds__(kTile* kTile) k_denoise_prepare_tiled(const float* rgb, const float4* albedo, const float4* normal, int width,
                                                                         int height, DenoiseConsts k, DenoiseBuffers buf) {
    constexpr int T = kTile + 2 * kVarRadius;
    __shared__ float4 sColour[T * T], sGuide[T * T];
    const int ox = blockIdx.x * kTile - kVarRadius, oy = blockIdx.y * kTile - kVarRadius;
    for (int t = threadIdx.y * kTile + threadIdx.x; t < T * T; t += kTile * kTile) {
        const int qx = ox + t % T, qy = oy + t / T;
        Pixel px;
        px.colour = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        px.guide = missGuide();
        if (qx >= 0 && qy >= 0 && qx < width && qy < height) px = decodePixel(rgb, albedo, normal, static_cast<size_t>(qy) * width + qx, k.demodulate);
        sColour[t] = px.colour;
        sGuide[t] = px.guide;
    }
    __syncthreads();
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    preparePixel(x, y, width, height, k, buf, [&](int qx, int qy) {
        const int t = (qy - oy) * T + (qx - ox);
        return Pixel{sColour[t], sGuide[t]};
    });
}

template <int S>
__global__ void __launch_bounds__(kTile* kTile) k_denoise_atrous_tiled(int width, int height, DenoiseConsts k, const float4* src, const float4* guide,
                                                                        const float* slopes, float4* dst) {
    constexpr int T = kTile + 2 * kTapRadius * S;
    static_assert(T * T * 2 * sizeof(float4) <= 32768, "tile plus halo must fit 32 KB of LDS");
    __shared__ float4 sColour[T * T], sGuide[T * T];
    const int ox = blockIdx.x * kTile - kTapRadius * S, oy = blockIdx.y * kTile - kTapRadius * S;
    for (int t = threadIdx.y * kTile + threadIdx.x; t < T * T; t += kTile * kTile) {
        const int qx = ox + t % T, qy = oy + t / T;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = missGuide();
        if (qx >= 0 && qy >= 0 && qx < width && qy < height) {
            const size_t q = static_cast<size_t>(qy) * width + qx;
            g = guide[q];
            if (g.w > 0.0f) c = src[q];   // a miss pixel's colour entry was never written
        }
        sColour[t] = c;
        sGuide[t] = g;
    }
    __syncthreads();
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    atrousPixel(x, y, width, height, S, k, slopes, dst, [&](int qx, int qy, float4& c, float4& g) {
        const int t = (qy - oy) * T + (qx - ox);
        c = sColour[t];
        g = sGuide[t];
    });
}

__global__ void __launch_bounds__(kTile* kTile) k_denoise_finish(const float* rgb, const float4* albedo, int width, int height, DenoiseConsts k,
                                                                  const float4* colour, const float4* guide, float* out) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t i = static_cast<size_t>(y) * width + x;
    float r = rgb[i * 3 + 0], g = rgb[i * 3 + 1], b = rgb[i * 3 + 2];   // (out may be rgb: a pixel is read and written by this thread alone)
    if (guide[i].w > 0.0f) {
        const float4 c = colour[i];
        const float3 a = albedoDivisor(albedo[i], k.demodulate);
        r = c.x * a.x;
        g = c.y * a.y;
        b = c.z * a.z;
    }
    out[i * 3 + 0] = r;
    out[i * 3 + 1] = g;
    out[i * 3 + 2] = b;
}

dim3 gridOf(uint32_t width, uint32_t height) { return dim3((width + kTile - 1) / kTile, (height + kTile - 1) / kTile); }

}  // namespace

void launchDenoisePrepare(const float* dRgb, const float4* dAlbedo, const float4* dNormal, uint32_t width, uint32_t height,
                          const PtrDenoiseParams& p, const DenoiseBuffers& buf, bool tiled, hipStream_t stream) {
    const dim3 grid = gridOf(width, height), block(kTile, kTile);
    const int w = static_cast<int>(width), h = static_cast<int>(height);
    if (tiled) {
        hipLaunchKernelGGL(k_denoise_prepare_tiled, grid, block, 0, stream, dRgb, dAlbedo, dNormal, w, h, constsOf(p), buf);
    } else {
        hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, stream, dRgb, dAlbedo, dNormal, w, h, constsOf(p), buf);
    }
}

void launchDenoisePrepareCov(const float* dRgb, const float4* dAlbedo, const float4* dNormal, const float* dCov, uint32_t width, uint32_t height,
                             const PtrDenoiseParams& p, const DenoiseBuffers& buf, hipStream_t stream) {
    hipLaunchKernelGGL(k_denoise_prepare_cov, gridOf(width, height), dim3(kTile, kTile), 0, stream, dRgb, dAlbedo, dNormal, dCov,
                       static_cast<int>(width), static_cast<int>(height), constsOf(p), buf);
}

void launchDenoiseAtrous(uint32_t width, uint32_t height, uint32_t step, const PtrDenoiseParams& p, const DenoiseBuffers& buf, uint32_t src,
                         bool tiled, hipStream_t stream) {
    const dim3 grid = gridOf(width, height), block(kTile, kTile);
    const int w = static_cast<int>(width), h = static_cast<int>(height);
    const float4* from = buf.colour[src];
    float4* to = buf.colour[src ^ 1u];
    const DenoiseConsts k = constsOf(p);
    if (tiled && step == 1u) {
        hipLaunchKernelGGL(k_denoise_atrous_tiled<1>, grid, block, 0, stream, w, h, k, from, buf.guide, buf.slope, to);
    } else if (tiled && step == 2u) {
        hipLaunchKernelGGL(k_denoise_atrous_tiled<2>, grid, block, 0, stream, w, h, k, from, buf.guide, buf.slope, to);
    } else if (tiled && step == 4u) {
        hipLaunchKernelGGL(k_denoise_atrous_tiled<4>, grid, block, 0, stream, w, h, k, from, buf.guide, buf.slope, to);
    } else {
        hipLaunchKernelGGL(k_denoise_atrous, grid, block, 0, stream, w, h, static_cast<int>(step), k, from, buf.guide, buf.slope, to);
    }
}

void launchDenoiseFinish(const float* dRgb, const float4* dAlbedo, uint32_t width, uint32_t height, const PtrDenoiseParams& p,
                         const DenoiseBuffers& buf, uint32_t src, float* dOut, hipStream_t stream) {
    hipLaunchKernelGGL(k_denoise_finish, gridOf(width, height), dim3(kTile, kTile), 0, stream, dRgb, dAlbedo, static_cast<int>(width),
                       static_cast<int>(height), constsOf(p), buf.colour[src], buf.guide, dOut);
}

}  // namespace ptrk
