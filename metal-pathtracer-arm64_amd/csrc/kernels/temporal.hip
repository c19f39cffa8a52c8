// Temporal accumulation: k_temporal_accumulate blends a frame's colour with the history of the surface point each pixel shows.
// The rule is spelled out in include/ptr_temporal.h; this file follows that text step by step (float32, unfused: the Makefile compiles it
// with -ffp-contract=off, in the order written), and so does the numpy restatement the tests compare it with (tests/temporal_ref.py).
//
// Image space only: 256-thread blocks, one pixel per lane, consecutive lanes on consecutive pixels of a row.  A lane streams its own
// three records (3 x 16 B), its colour (12 B) and its outputs (12 B + 4 B + 16 B), and gathers up to four taps of three 16 B loads each
// (previous R0, previous R1, history), which neighbouring lanes mostly share.  No LDS, no atomics, nothing passes between workgroups:
// the history is read from one buffer and written to the other.
#include <hip/hip_runtime.h>

#include "temporal.h"
#include "vec.h"

namespace ptrk {

namespace {

constexpr uint32_t kTemporalBlock = 256u;
constexpr uint32_t kMissWord = 0xFFFFFFFFu;   // bvh_layout.h kHitMiss

struct Cam {
    f3 o, ll, h, w;
};

Cam camOf(const TemporalCamera& c) {
    return Cam{f3{c.o[0], c.o[1], c.o[2]}, f3{c.ll[0], c.ll[1], c.ll[2]}, f3{c.h[0], c.h[1], c.h[2]}, f3{c.w[0], c.w[1], c.w[2]}};
}

// step 3: where the camera sees Y, in pixels; false when Y is behind the camera or in its plane
__device__ __forceinline__ bool project(const Cam& cam, f3 y, float width, float height, float& fx, float& fy) {
    const f3 d = y - cam.o;
    const f3 cN = cross(cam.h, cam.w);
    const f3 L = cam.ll - cam.o;
    const float den = dot(d, cN);
    const float num = dot(L, cN);
    const float s = num / den;
    if (!(s > 0.0f && __builtin_isfinite(s))) return false;
    const f3 r = d * s - L;
    const float U = dot(r, cam.h) / dot(cam.h, cam.h);
    const float V = dot(r, cam.w) / dot(cam.w, cam.w);
    fx = U * width;
    fy = (1.0f - V) * height;
    return true;
}

__global__ void __launch_bounds__(kTemporalBlock) k_temporal_accumulate(const float* rgb, TemporalBuffers buf, Cam cur, Cam prev,
                                                                         uint32_t width, uint32_t height, float maxHistory, float normalCos,
                                                                         float planeTolerance, uint32_t hasHistory, float* out, float* outLength) {
    const uint32_t i = blockIdx.x * kTemporalBlock + threadIdx.x;
    if (i >= width * height) return;
    const size_t at = static_cast<size_t>(i) * 3u;
    const f3 c = mk3(rgb[at], rgb[at + 1u], rgb[at + 2u]);   // (read before `out`, which may be the same buffer, is written)
    const float4 r0 = buf.r0[i], r2 = buf.r2[i];
    f3 result = c;
    float length = 1.0f;
    if (__float_as_uint(r2.w) == kMissWord || !finite3(c)) {
        length = 0.0f;   // step 1
    } else if (hasHistory) {
        const float4 r1 = buf.r1[i];
        const f3 xPrev = mk3(r2), n = mk3(r1);
        const float w = static_cast<float>(width), h = static_cast<float>(height);
        float fcx, fcy, fpx, fpy;
        if (project(cur, mk3(r0), w, h, fcx, fcy) && project(prev, xPrev, w, h, fpx, fpy)) {
            const uint32_t px = i % width, py = i / width;
            const float sx = static_cast<float>(px) + (fpx - fcx), sy = static_cast<float>(py) + (fpy - fcy);
            if (__builtin_isfinite(sx) && __builtin_isfinite(sy)) {
                const float x0 = floorf(sx), y0 = floorf(sy);
                const float ax = sx - x0, ay = sy - y0;
                const float bx[2] = {1.0f - ax, ax}, by[2] = {1.0f - ay, ay};
                const f3 toCamera = xPrev - prev.o;
                const float bound = planeTolerance * sqrtf(dot(toCamera, toCamera));
                float B = 0.0f, Sn = 0.0f;
                f3 Sc = mk3(0.0f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float b = bx[k & 1] * by[k >> 1];
                    const float tx = x0 + static_cast<float>(k & 1), ty = y0 + static_cast<float>(k >> 1);
                    if (!(b > 0.0f && tx >= 0.0f && tx < w && ty >= 0.0f && ty < h)) continue;
                    const uint32_t q = static_cast<uint32_t>(ty) * width + static_cast<uint32_t>(tx);
                    const float4 hq = buf.history[q], q0 = buf.prevR0[q], q1 = buf.prevR1[q];
                    const f3 nq = mk3(q1);
                    const bool counts = hq.w >= 1.0f && finite3(mk3(hq)) && __float_as_uint(q0.w) == __float_as_uint(r0.w) &&
                                        dot(nq, n) >= normalCos && fabsf(dot(xPrev - mk3(q0), nq)) <= bound;
                    if (!counts) continue;
                    B = B + b;
                    Sc = Sc + b * mk3(hq);
                    Sn = Sn + b * hq.w;
                }
                if (B > 0.0f) {
                    const f3 hist = Sc / B;
                    const float N = Sn / B;
                    const float grown = N + 1.0f;
                    length = grown < maxHistory ? grown : maxHistory;
                    const float a = 1.0f / length;
                    result = hist + (c - hist) * a;
                }
            }
        }
    }
    buf.historyOut[i] = mk4(result, length);
    out[at] = result.x;
    out[at + 1u] = result.y;
    out[at + 2u] = result.z;
    if (outLength) outLength[i] = length;
}

}  // namespace

void launchTemporalAccumulate(const float* dRgb, const TemporalBuffers& buf, const TemporalCamera& cur, const TemporalCamera& prev, uint32_t width,
                              uint32_t height, const PtrTemporalParams& p, bool hasHistory, float* dOut, float* dLength, hipStream_t stream) {
    const uint32_t pixels = width * height;
    hipLaunchKernelGGL(k_temporal_accumulate, dim3((pixels + kTemporalBlock - 1u) / kTemporalBlock), dim3(kTemporalBlock), 0, stream, dRgb, buf,
                       camOf(cur), camOf(prev), width, height, static_cast<float>(p.maxHistory), p.normalCos, p.planeTolerance, hasHistory ? 1u : 0u,
                       dOut, dLength);
}

}  // namespace ptrk
