// Host-callable launchers of the denoiser kernels (defined in denoise.hip; the filter itself is spelled out in include/ptr_post.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptr_post.h"

namespace ptrk {

// Scratch of one denoise call, width*height entries each.
struct DenoiseBuffers {
    float4* colour[2];   // demodulated colour rgb | variance, ping-pong (prepare writes [0])
    float4* guide;       // unit normal xyz | depth z; z <= 0 marks a miss pixel
    float* slope;        // depth slope g_p
};

// The a-trous steps that have an LDS-tiled kernel: tile plus halo (16 + 4 s)^2 * 32 B <= 32 KB.
constexpr uint32_t kDenoiseMaxTiledStep = 4u;

// tiled: stage the block's pixels and their halo in LDS instead of reading every tap through the caches.  Same arithmetic in the
// same order: the two variants give the same bits.
void launchDenoisePrepare(const float* dRgb, const float4* dAlbedo, const float4* dNormal, uint32_t width, uint32_t height,
                          const PtrDenoiseParams& p, const DenoiseBuffers& buf, bool tiled, hipStream_t stream);
// prepare with the variance taken from dCov (width*height*6 floats; include/ptr_stats.h) instead of the 7x7 spatial estimate.  Simple
// variant only (nine taps).
void launchDenoisePrepareCov(const float* dRgb, const float4* dAlbedo, const float4* dNormal, const float* dCov, uint32_t width, uint32_t height,
                             const PtrDenoiseParams& p, const DenoiseBuffers& buf, hipStream_t stream);
// pass at step `step` (a power of two) from buf.colour[src] to buf.colour[src ^ 1]; tiled needs step <= kDenoiseMaxTiledStep
void launchDenoiseAtrous(uint32_t width, uint32_t height, uint32_t step, const PtrDenoiseParams& p, const DenoiseBuffers& buf, uint32_t src,
                         bool tiled, hipStream_t stream);
// dOut may equal dRgb
void launchDenoiseFinish(const float* dRgb, const float4* dAlbedo, uint32_t width, uint32_t height, const PtrDenoiseParams& p,
                         const DenoiseBuffers& buf, uint32_t src, float* dOut, hipStream_t stream);

}  // namespace ptrk
