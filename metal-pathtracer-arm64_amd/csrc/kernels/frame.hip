// The kernels a resumable frame adds between the rounds of a refine (include/ptr_frame.h; the per-element bodies are in frame.h).  Compiled
// like adaptive.hip, unfused with correctly rounded division; everything that touches a sample value is adaptive.hip's own kernel.
//
// k_frame_class_min: one thread per entry j of L; the minimum of n over a wave by shuffles, over the block through LDS, and one vector
// atomicMin per block on the result word (the value does not depend on the order the blocks arrive in).
// k_frame_split: the flag "n == n_min" per entry and its count per 256-thread block (ballot + popcount, as k_adaptive_select); the scan
// and the scatter that follow are adaptive.hip's, so S keeps L's order.
// k_frame_merge: the flag "not in S, or Select keeps it" per entry of L and its count per block; the same scan and scatter give the next L.
// No atomics decide a position.
#include <hip/hip_runtime.h>

#include "frame.h"

namespace ptrk {

namespace {

constexpr uint32_t kBlock = kCompactBlock;
constexpr uint32_t kWaves = kCompactWaves;

__global__ void __launch_bounds__(kBlock) k_frame_class_min(const uint32_t* __restrict__ list, uint32_t count, const uint32_t* __restrict__ n,
                                                            uint32_t* __restrict__ result) {
    __shared__ uint32_t waveMin[kWaves];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    uint32_t low = kFrameNoCount;
    if (j < count) low = frameClassMin(low, list, j, n);
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(low), step, 64));
        low = other < low ? other : low;
    }
    if ((threadIdx.x & 63u) == 0u) waveMin[threadIdx.x >> 6] = low;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t w = 1; w < kWaves; ++w) low = waveMin[w] < low ? waveMin[w] : low;
        atomicMin(result, low);
    }
}

__global__ void __launch_bounds__(kBlock) k_frame_split(const uint32_t* __restrict__ list, uint32_t count, const uint32_t* __restrict__ n, uint32_t nMin,
                                                        uint8_t* __restrict__ inS, uint32_t* __restrict__ blockCounts) {
    __shared__ uint32_t waveCounts[kWaves];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool keep = false;
    if (j < count) {
        keep = frameInClass(list, j, n, nMin);
        inS[j] = keep ? 1u : 0u;
    }
    uint32_t total;
    (void)blockRank(keep, waveCounts, total);
    if (threadIdx.x == 0u) blockCounts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock) k_frame_merge(const uint32_t* __restrict__ list, uint32_t count, const uint8_t* __restrict__ inS, uint32_t width,
                                                        uint32_t height, const float* __restrict__ e, const uint32_t* __restrict__ n, uint32_t maxSpp,
                                                        float threshold, uint8_t* __restrict__ keepOut, uint32_t* __restrict__ blockCounts) {
    __shared__ uint32_t waveCounts[kWaves];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool keep = false;
    if (j < count) {
        keep = frameMergeKeep(list, j, inS, width, height, e, n, maxSpp, threshold);
        keepOut[j] = keep ? 1u : 0u;
    }
    uint32_t total;
    (void)blockRank(keep, waveCounts, total);
    if (threadIdx.x == 0u) blockCounts[blockIdx.x] = total;
}

uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

}  // namespace

void launchFrameClassMin(const uint32_t* dList, uint32_t count, const uint32_t* dN, uint32_t* dMin, hipStream_t stream) {
    const uint32_t blocks = blocksFor(count);
    if (blocks > 0u) hipLaunchKernelGGL(k_frame_class_min, dim3(blocks), dim3(kBlock), 0, stream, dList, count, dN, dMin);
}

void launchFrameSplit(const uint32_t* dList, uint32_t count, const uint32_t* dN, uint32_t nMin, uint8_t* dInS, const AdaptiveScratch& scratch,
                      uint32_t* dS, hipStream_t stream) {
    const uint32_t blocks = blocksFor(count);
    if (blocks > 0u) hipLaunchKernelGGL(k_frame_split, dim3(blocks), dim3(kBlock), 0, stream, dList, count, dN, nMin, dInS, scratch.blockCounts);
    launchAdaptiveCompact(dList, count, dInS, scratch, dS, stream);
}

void launchFrameMerge(const uint32_t* dList, uint32_t count, const uint8_t* dInS, uint32_t width, uint32_t height, const AdaptiveState& state,
                      uint32_t maxSpp, float threshold, const AdaptiveScratch& scratch, uint32_t* dNext, hipStream_t stream) {
    const uint32_t blocks = blocksFor(count);
    if (blocks > 0u) {
        hipLaunchKernelGGL(k_frame_merge, dim3(blocks), dim3(kBlock), 0, stream, dList, count, dInS, width, height, state.e, state.n, maxSpp, threshold,
                           scratch.keep, scratch.blockCounts);
    }
    launchAdaptiveCompact(dList, count, scratch.keep, scratch, dNext, stream);
}

}  // namespace ptrk
