// The kernels of the frames on several devices (include/ptr_multi.h, and the gather of ptr_render_multi; the per-element bodies are in multi.h).
// Compiled like adaptive.hip, unfused with correctly rounded division: k_multi_finish_bands has to give the bits of k_adaptive_finish.
//
// k_multi_halo_pack / k_multi_halo_unpack: one thread per float of the partition's edge rows; consecutive threads walk a row, so a wave
// reads (pack) or writes (unpack) 256 contiguous bytes of the e image unless it straddles the end of a row.
// k_multi_finish_bands: one thread per pixel position of the partition's band layout.
// k_multi_interleave: one thread per 4-byte word of the image, the gather step of every multi-device frame, for 3, 6 or 1 words per pixel.
// k_multi_gather_items (probe only): one thread per (sample, list entry).
// k_multi_state_pack / k_multi_state_unpack (include/ptr_multi_frame.h): one thread per pixel position of the partition's band layout.
// Consecutive threads walk an image row, and a band's rows are contiguous in the image, so a wave reads (pack) or writes (unpack) one
// contiguous run of each image-order array - 768 / 768 / 1536 / 256 / 256 bytes of sum / mean / M / n / e - and the same run of each
// plane; only a wave that straddles the end of a band touches two runs.  Streaming copies: 56 bytes in, 56 out per pixel, no reuse.
#include <hip/hip_runtime.h>

#include "multi.h"

namespace ptrk {

namespace {

constexpr uint32_t kBlock = 256u;

__global__ void __launch_bounds__(kBlock) k_multi_halo_pack(MultiPart mp, const float* __restrict__ e, float* __restrict__ edge) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.bands * 2u * mp.width) return;
    multiHaloPack(mp, i, e, edge);
}

__global__ void __launch_bounds__(kBlock) k_multi_halo_unpack(MultiPart mp, const float* __restrict__ edge, float* __restrict__ e) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.bands * 2u * mp.width) return;
    multiHaloUnpack(mp, i, edge, e);
}

__global__ void __launch_bounds__(kBlock) k_multi_finish_bands(MultiPart mp, AdaptiveState st, float* __restrict__ rgb, float* __restrict__ cov,
                                                               uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.bands * kMultiBandRows * mp.width) return;
    multiFinishBands(mp, i, st, rgb, cov, count);
}

__global__ void __launch_bounds__(kBlock) k_multi_interleave(const uint32_t* __restrict__ gathered, const uint64_t* __restrict__ partWordOffset,
                                                             uint32_t parts, uint32_t width, uint32_t height, uint32_t channels,
                                                             uint32_t* __restrict__ image) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= static_cast<uint64_t>(width) * channels * height) return;
    multiInterleave(i, gathered, partWordOffset, parts, width, channels, image);
}

__global__ void __launch_bounds__(kBlock) k_multi_gather_items(const float4* __restrict__ samples, size_t pixels, const uint32_t* __restrict__ list,
                                                               uint32_t active, uint32_t spp, uint32_t nBefore, float4* __restrict__ items) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= static_cast<uint64_t>(active) * spp) return;
    const uint32_t c = static_cast<uint32_t>(i / active), j = static_cast<uint32_t>(i - static_cast<uint64_t>(c) * active);
    items[i] = samples[static_cast<size_t>(nBefore + c) * pixels + list[j]];
}

__global__ void __launch_bounds__(kBlock) k_multi_state_pack(MultiPart mp, AdaptiveState st, float* __restrict__ packed) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.bands * kMultiBandRows * mp.width) return;
    multiStatePack(mp, i, st, packed);
}

__global__ void __launch_bounds__(kBlock) k_multi_state_unpack(MultiPart mp, const float* __restrict__ packed, AdaptiveState st) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.bands * kMultiBandRows * mp.width) return;
    multiStateUnpack(mp, i, packed, st);
}

uint32_t blocksFor(uint64_t n) { return static_cast<uint32_t>((n + kBlock - 1u) / kBlock); }

}  // namespace

void launchMultiStatePack(const MultiPart& mp, const AdaptiveState& state, float* dPacked, hipStream_t stream) {
    const uint32_t blocks = blocksFor(multiBandPixels(mp));
    if (blocks) hipLaunchKernelGGL(k_multi_state_pack, dim3(blocks), dim3(kBlock), 0, stream, mp, state, dPacked);
}

void launchMultiStateUnpack(const MultiPart& mp, const float* dPacked, const AdaptiveState& state, hipStream_t stream) {
    const uint32_t blocks = blocksFor(multiBandPixels(mp));
    if (blocks) hipLaunchKernelGGL(k_multi_state_unpack, dim3(blocks), dim3(kBlock), 0, stream, mp, dPacked, state);
}

void launchMultiHaloPack(const MultiPart& mp, const float* dE, float* dEdge, hipStream_t stream) {
    const uint32_t blocks = blocksFor(static_cast<uint64_t>(mp.bands) * 2u * mp.width);
    if (blocks) hipLaunchKernelGGL(k_multi_halo_pack, dim3(blocks), dim3(kBlock), 0, stream, mp, dE, dEdge);
}

void launchMultiHaloUnpack(const MultiPart& mp, const float* dEdge, float* dE, hipStream_t stream) {
    const uint32_t blocks = blocksFor(static_cast<uint64_t>(mp.bands) * 2u * mp.width);
    if (blocks) hipLaunchKernelGGL(k_multi_halo_unpack, dim3(blocks), dim3(kBlock), 0, stream, mp, dEdge, dE);
}

void launchMultiFinishBands(const MultiPart& mp, const AdaptiveState& state, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    const uint32_t blocks = blocksFor(static_cast<uint64_t>(mp.bands) * kMultiBandRows * mp.width);
    if (blocks) hipLaunchKernelGGL(k_multi_finish_bands, dim3(blocks), dim3(kBlock), 0, stream, mp, state, dRgb, dCov, dCount);
}

void launchMultiInterleave(const void* dGathered, const uint64_t* dPartWordOffset, uint32_t parts, uint32_t width, uint32_t height, uint32_t channels,
                           void* dImage, hipStream_t stream) {
    const uint32_t blocks = blocksFor(static_cast<uint64_t>(width) * channels * height);
    if (blocks) {
        hipLaunchKernelGGL(k_multi_interleave, dim3(blocks), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(dGathered), dPartWordOffset, parts, width,
                           height, channels, static_cast<uint32_t*>(dImage));
    }
}

void launchMultiGatherItems(const float4* dSamples, size_t pixels, const uint32_t* dList, uint32_t active, uint32_t spp, uint32_t nBefore, float4* dItems,
                            hipStream_t stream) {
    const uint32_t blocks = blocksFor(static_cast<uint64_t>(active) * spp);
    if (blocks) hipLaunchKernelGGL(k_multi_gather_items, dim3(blocks), dim3(kBlock), 0, stream, dSamples, pixels, dList, active, spp, nBefore, dItems);
}

}  // namespace ptrk
