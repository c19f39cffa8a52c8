// Host-callable launchers of the temporal accumulation kernels (defined in temporal.hip; the rules are spelled out in
// include/ptr_temporal.h and include/ptr_temporal_cov.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ptr_temporal.h"

namespace ptrk {

// A camera as the filter projects through it: origin, lower-left corner, horizontal, vertical (CameraParams' first four fields).
struct TemporalCamera {
    float o[3], ll[3], h[3], w[3];
};

// The buffers of one step, width*height entries each.
struct TemporalBuffers {
    const float4* r0;        // this step's records
    const float4* r1;
    const float4* r2;
    const float4* prevR0;    // the previous step's (never read without history)
    const float4* prevR1;
    const float4* history;   // (rgb, length) of the previous step (never read without history)
    float4* historyOut;      // a different buffer from `history`: a lane reads four taps other lanes write
};

// dOut may equal dRgb; dLength may be null
void launchTemporalAccumulate(const float* dRgb, const TemporalBuffers& buf, const TemporalCamera& cur, const TemporalCamera& prev, uint32_t width,
                              uint32_t height, const PtrTemporalParams& p, bool hasHistory, float* dOut, float* dLength, hipStream_t stream);

// What k_temporal_accumulate_cov (include/ptr_temporal_cov.h) takes beside those: six floats per pixel each.  cov and outCov are in image
// order and 8 B aligned; a covariance history is 24 B per pixel in two planes, (rr, gg, bb, rg) of every pixel, then (rb, gb) of every pixel.
struct TemporalCovBuffers {
    const float* cov;
    float* outCov;          // may equal cov
    const float* history;   // never read without history
    float* historyOut;      // a different buffer from `history`
};

inline float4* covPlaneA(float* history, size_t) { return reinterpret_cast<float4*>(history); }
inline const float4* covPlaneA(const float* history, size_t) { return reinterpret_cast<const float4*>(history); }
inline float2* covPlaneB(float* history, size_t pixels) { return reinterpret_cast<float2*>(history + 4u * pixels); }
inline const float2* covPlaneB(const float* history, size_t pixels) { return reinterpret_cast<const float2*>(history + 4u * pixels); }

void launchTemporalAccumulateCov(const float* dRgb, const TemporalBuffers& buf, const TemporalCovBuffers& cov, const TemporalCamera& cur,
                                 const TemporalCamera& prev, uint32_t width, uint32_t height, const PtrTemporalParams& p, float rejectSigma,
                                 bool hasHistory, float* dOut, float* dLength, hipStream_t stream);

}  // namespace ptrk
