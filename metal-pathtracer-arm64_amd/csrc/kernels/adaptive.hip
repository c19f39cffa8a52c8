// The kernels that run between the rounds of an adaptive frame (include/ptr_adaptive.h; the per-element bodies are in adaptive.h).  Like
// stats.hip this file is compiled unfused (-ffp-contract=off) with correctly rounded division and square root; the numpy restatement
// the tests compare it with is tests/adaptive_ref.py.
//
// k_adaptive_update: one thread per entry j of the active list.  Sample c of entry j is item c * activeCount + j, so a wave reads 1 KiB
// contiguous per sample; the loads do not depend on the recurrence and four are issued before the first is consumed (as k_resolve_cov).
// The state lives at pixel = list[j], in image order.
// k_adaptive_select -> k_adaptive_scan -> k_adaptive_scatter: a keep flag per entry, counted per 256-thread block with a wave ballot and
// a popcount; one block scans the per-block counts (8,100 of them at 1080p); the scatter recomputes each entry's rank inside its block
// from the ballot's bits below the lane and writes the next list.  No atomics: the order is the current list's.
#include <hip/hip_runtime.h>

#include "adaptive.h"

namespace ptrk {

namespace {

constexpr uint32_t kUpdateUnroll = 4u;
constexpr uint32_t kBlock = kCompactBlock;
constexpr uint32_t kWaves = kCompactWaves;

__global__ void __launch_bounds__(kBlock) k_adaptive_update(const float4* __restrict__ items, const uint32_t* __restrict__ list, uint32_t activeCount,
                                                            uint32_t spp, uint32_t nBefore, uint32_t last, AdaptiveState st) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= activeCount) return;
    const uint32_t pixel = list[j];
    AdaptivePixel p;
    p.load(st, pixel);
    const float4* mine = items + j;
    const size_t stride = activeCount;
    uint32_t c = 0;
    for (; c + kUpdateUnroll <= spp; c += kUpdateUnroll) {
        float4 xs[kUpdateUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUpdateUnroll; ++u) xs[u] = mine[static_cast<size_t>(c + u) * stride];
#pragma unroll
        for (uint32_t u = 0; u < kUpdateUnroll; ++u) p.add(xs[u].x, xs[u].y, xs[u].z, nBefore + c + u + 1u);
    }
    for (; c < spp; ++c) {
        const float4 x = mine[static_cast<size_t>(c) * stride];
        p.add(x.x, x.y, x.z, nBefore + c + 1u);
    }
    p.store(st, pixel);
    const uint32_t n = nBefore + spp;
    st.n[pixel] = n;
    if (last) st.e[pixel] = p.error(n);
}

__global__ void __launch_bounds__(kBlock) k_adaptive_select(const uint32_t* __restrict__ list, uint32_t activeCount, uint32_t width, uint32_t height,
                                                            const float* __restrict__ e, const uint32_t* __restrict__ n, uint32_t maxSpp,
                                                            float threshold, uint8_t* __restrict__ keepOut, uint32_t* __restrict__ blockCounts) {
    __shared__ uint32_t waveCounts[kWaves];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool keep = false;
    if (j < activeCount) {
        keep = adaptiveKeep(list[j], width, height, e, n, maxSpp, threshold);
        keepOut[j] = keep ? 1u : 0u;
    }
    uint32_t total;
    (void)blockRank(keep, waveCounts, total);
    if (threadIdx.x == 0u) blockCounts[blockIdx.x] = total;
}

// One block: offsets[b] = counts[0] + .. + counts[b - 1], *total = the sum of all.
__global__ void __launch_bounds__(kBlock) k_adaptive_scan(const uint32_t* __restrict__ counts, uint32_t blocks, uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ total) {
    __shared__ uint32_t part[kBlock];
    uint32_t running = 0u;
    for (uint32_t base = 0; base < blocks; base += kBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t mine = b < blocks ? counts[b] : 0u;
        part[threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t step = 1u; step < kBlock; step <<= 1) {   // inclusive scan of the chunk
            const uint32_t add = threadIdx.x >= step ? part[threadIdx.x - step] : 0u;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < blocks) offsets[b] = running + part[threadIdx.x] - mine;
        running += part[kBlock - 1u];
        __syncthreads();   // part is rewritten by the next chunk
    }
    if (threadIdx.x == 0u) *total = running;
}

__global__ void __launch_bounds__(kBlock) k_adaptive_scatter(const uint32_t* __restrict__ list, uint32_t activeCount, const uint8_t* __restrict__ keepIn,
                                                             const uint32_t* __restrict__ blockOffsets, uint32_t* __restrict__ next) {
    __shared__ uint32_t waveCounts[kWaves];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = j < activeCount && keepIn[j] != 0u;
    uint32_t total;
    const uint32_t rank = blockRank(keep, waveCounts, total);
    if (keep) next[blockOffsets[blockIdx.x] + rank] = list[j];   // rank < the block's count: the index stays below the total <= activeCount
}

__global__ void __launch_bounds__(kBlock) k_adaptive_finish(AdaptiveState st, uint32_t pixels, float* __restrict__ rgb, float* __restrict__ cov,
                                                            uint32_t* __restrict__ count) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t n = st.n[p];
    const float fn = static_cast<float>(n);
    const float* s = st.sum + static_cast<size_t>(p) * 3u;
    float* o = rgb + static_cast<size_t>(p) * 3u;
    o[0] = s[0] / fn;
    o[1] = s[1] / fn;
    o[2] = s[2] / fn;
    if (cov) {
        const float norm = fn * static_cast<float>(n - 1u);
        const float* m = st.m + static_cast<size_t>(p) * 6u;
        float* c = cov + static_cast<size_t>(p) * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) c[k] = m[k] / norm;
    }
    if (count) count[p] = n;
}

uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

}  // namespace

void launchAdaptiveUpdate(const float4* dItems, const uint32_t* dList, uint32_t activeCount, uint32_t spp, uint32_t nBefore, bool last,
                          const AdaptiveState& state, hipStream_t stream) {
    if (activeCount == 0u) return;
    hipLaunchKernelGGL(k_adaptive_update, dim3(blocksFor(activeCount)), dim3(kBlock), 0, stream, dItems, dList, activeCount, spp, nBefore, last ? 1u : 0u,
                       state);
}

void launchAdaptiveSelect(const uint32_t* dList, uint32_t activeCount, uint32_t width, uint32_t height, const AdaptiveState& state, uint32_t maxSpp,
                          float threshold, const AdaptiveScratch& scratch, uint32_t* dNext, hipStream_t stream) {
    const uint32_t blocks = blocksFor(activeCount);
    if (blocks > 0u) {
        hipLaunchKernelGGL(k_adaptive_select, dim3(blocks), dim3(kBlock), 0, stream, dList, activeCount, width, height, state.e, state.n, maxSpp, threshold,
                           scratch.keep, scratch.blockCounts);
    }
    launchAdaptiveCompact(dList, activeCount, scratch.keep, scratch, dNext, stream);
}

void launchAdaptiveCompact(const uint32_t* dList, uint32_t activeCount, const uint8_t* dKeep, const AdaptiveScratch& scratch, uint32_t* dNext,
                           hipStream_t stream) {
    const uint32_t blocks = blocksFor(activeCount);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kBlock), 0, stream, scratch.blockCounts, blocks, scratch.blockOffsets, scratch.total);
    if (blocks > 0u) {
        hipLaunchKernelGGL(k_adaptive_scatter, dim3(blocks), dim3(kBlock), 0, stream, dList, activeCount, dKeep, scratch.blockOffsets, dNext);
    }
}

void launchAdaptiveFinish(const AdaptiveState& state, uint32_t pixels, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    hipLaunchKernelGGL(k_adaptive_finish, dim3(blocksFor(pixels)), dim3(kBlock), 0, stream, state, pixels, dRgb, dCov, dCount);
}

}  // namespace ptrk
