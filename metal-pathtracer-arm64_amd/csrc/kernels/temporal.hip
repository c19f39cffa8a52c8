// Temporal accumulation: k_temporal_accumulate blends a frame's colour with the history of the surface point each pixel shows.
// The rule is spelled out in include/ptr_temporal.h; this file follows that text step by step (float32, unfused: the Makefile compiles it
// with -ffp-contract=off, in the order written), and so does the numpy restatement the tests compare it with (tests/temporal_ref.py).
//
// Image space only: 256-thread blocks, one pixel per lane, consecutive lanes on consecutive pixels of a row.  A lane streams its own
// three records (3 x 16 B), its colour (12 B) and its outputs (12 B + 4 B + 16 B), and gathers up to four taps of three 16 B loads each
// (previous R0, previous R1, history), which neighbouring lanes mostly share.  No LDS, no atomics, nothing passes between workgroups:
// the history is read from one buffer and written to the other.
//
// k_temporal_accumulate_cov is the same body (temporal_pixel.inc) with the covariance rule of include/ptr_temporal_cov.h compiled in
// (restated in tests/temporal_cov_ref.py): a lane also streams its frame covariance (3 x 8 B), out_cov (3 x 8 B) and its covariance
// history (16 B + 8 B), 164 B of its own against 92 B, and a tap is 16 B + 8 B more, 72 B against 48 B.
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
#define PTR_TEMPORAL_COV 0
#include "temporal_pixel.inc"
#undef PTR_TEMPORAL_COV
}

// What the covariance rule (include/ptr_temporal_cov.h) adds to a pixel's inputs and outputs.  The frame's covariance and out_cov are six
// floats per pixel in image order, read and written as three 8 B pairs; a covariance history is two planes, (rr, gg, bb, rg) in 16 B and
// (rb, gb) in 8 B per pixel, so that a tap is one load of each.
struct CovIo {
    const float2* cov;        // may be the buffer outCov is
    float2* outCov;
    const float4* historyA;   // never read without history
    const float2* historyB;
    float4* historyAOut;      // different buffers from historyA / historyB, as historyOut is from history
    float2* historyBOut;
    float rejectSigma;
};

__device__ __forceinline__ float lum(f3 x) { return (0.2126f * x.x + 0.7152f * x.y) + 0.0722f * x.z; }

// C as (rr, gg, bb, rg, rb, gb)
__device__ __forceinline__ float lumvar(const float (&C)[6]) {
    constexpr float k[3] = {0.2126f, 0.7152f, 0.0722f};
    constexpr int at[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int d = 0; d < 3; ++d) v = v + (k[c] * k[d]) * C[at[c][d]];
    }
    return __builtin_isfinite(v) && v > 0.0f ? v : 0.0f;
}

__global__ void __launch_bounds__(kTemporalBlock) k_temporal_accumulate_cov(const float* rgb, TemporalBuffers buf, CovIo cv, Cam cur, Cam prev,
                                                                             uint32_t width, uint32_t height, float maxHistory, float normalCos,
                                                                             float planeTolerance, uint32_t hasHistory, float* out,
                                                                             float* outLength) {
#define PTR_TEMPORAL_COV 1
#include "temporal_pixel.inc"
#undef PTR_TEMPORAL_COV
}

}  // namespace

void launchTemporalAccumulate(const float* dRgb, const TemporalBuffers& buf, const TemporalCamera& cur, const TemporalCamera& prev, uint32_t width,
                              uint32_t height, const PtrTemporalParams& p, bool hasHistory, float* dOut, float* dLength, hipStream_t stream) {
    const uint32_t pixels = width * height;
    hipLaunchKernelGGL(k_temporal_accumulate, dim3((pixels + kTemporalBlock - 1u) / kTemporalBlock), dim3(kTemporalBlock), 0, stream, dRgb, buf,
                       camOf(cur), camOf(prev), width, height, static_cast<float>(p.maxHistory), p.normalCos, p.planeTolerance, hasHistory ? 1u : 0u,
                       dOut, dLength);
}

void launchTemporalAccumulateCov(const float* dRgb, const TemporalBuffers& buf, const TemporalCovBuffers& cov, const TemporalCamera& cur,
                                 const TemporalCamera& prev, uint32_t width, uint32_t height, const PtrTemporalParams& p, float rejectSigma,
                                 bool hasHistory, float* dOut, float* dLength, hipStream_t stream) {
    const uint32_t pixels = width * height;
    const CovIo cv{reinterpret_cast<const float2*>(cov.cov), reinterpret_cast<float2*>(cov.outCov), covPlaneA(cov.history, pixels),
                   covPlaneB(cov.history, pixels), covPlaneA(cov.historyOut, pixels), covPlaneB(cov.historyOut, pixels), rejectSigma};
    hipLaunchKernelGGL(k_temporal_accumulate_cov, dim3((pixels + kTemporalBlock - 1u) / kTemporalBlock), dim3(kTemporalBlock), 0, stream, dRgb, buf,
                       cv, camOf(cur), camOf(prev), width, height, static_cast<float>(p.maxHistory), p.normalCos, p.planeTolerance,
                       hasHistory ? 1u : 0u, dOut, dLength);
}

}  // namespace ptrk
