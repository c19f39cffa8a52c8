// Adaptive sampling between rounds (include/ptr_adaptive.h, whose text this file follows line by line): the per-element bodies of the
// kernels in adaptive.hip, written as host + device functions on plain pointers so that the renderer, the test-only probe and a host
// program that walks the index arithmetic all run the same code, and the launchers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTR_HD __host__ __device__ inline
#else
#include <math.h>
#define PTR_HD inline
#endif

namespace ptrk {

// The per-pixel state, image order (ptr_adaptive.h): sum / mean 3 floats, m 6 floats per pixel.
struct AdaptiveState {
    float* sum;
    float* mean;
    float* m;
    uint32_t* n;
    float* e;
};

// The running sums of one pixel while a round's samples are folded in.
struct AdaptivePixel {
    float sr, sg, sb;
    float mr, mg, mb;
    float rr, gg, bb, rg, rb, gb;
    PTR_HD void load(const AdaptiveState& st, uint32_t pixel) {
        const float* s = st.sum + static_cast<size_t>(pixel) * 3u;
        const float* a = st.mean + static_cast<size_t>(pixel) * 3u;
        const float* c = st.m + static_cast<size_t>(pixel) * 6u;
        sr = s[0], sg = s[1], sb = s[2];
        mr = a[0], mg = a[1], mb = a[2];
        rr = c[0], gg = c[1], bb = c[2], rg = c[3], rb = c[4], gb = c[5];
    }
    PTR_HD void store(const AdaptiveState& st, uint32_t pixel) const {
        float* s = st.sum + static_cast<size_t>(pixel) * 3u;
        float* a = st.mean + static_cast<size_t>(pixel) * 3u;
        float* c = st.m + static_cast<size_t>(pixel) * 6u;
        s[0] = sr, s[1] = sg, s[2] = sb;
        a[0] = mr, a[1] = mg, a[2] = mb;
        c[0] = rr, c[1] = gg, c[2] = bb, c[3] = rg, c[4] = rb, c[5] = gb;
    }
    // sample x, the k-th of the frame (1-based)
    PTR_HD void add(float xr, float xg, float xb, uint32_t k) {
        sr = sr + xr;
        sg = sg + xg;
        sb = sb + xb;
        const float fk = static_cast<float>(k);
        const float dr = xr - mr, dg = xg - mg, db = xb - mb;
        mr = mr + dr / fk;
        mg = mg + dg / fk;
        mb = mb + db / fk;
        const float er = xr - mr, eg = xg - mg, eb = xb - mb;
        rr += dr * er;
        gg += dg * eg;
        bb += db * eb;
        rg += dr * eg;
        rb += dr * eb;
        gb += dg * eb;
    }
    // the relative standard error of the mean's luminance after n samples
    PTR_HD float error(uint32_t n) const {
        const float norm = static_cast<float>(n) * static_cast<float>(n - 1u);
        const float c[3][3] = {{rr / norm, rg / norm, rb / norm}, {rg / norm, gg / norm, gb / norm}, {rb / norm, gb / norm, bb / norm}};
        const float k[3] = {0.2126f, 0.7152f, 0.0722f};
        float v = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) v = v + (k[a] * k[b]) * c[a][b];
        }
        if (!(__builtin_isfinite(v) && v > 0.0f)) v = 0.0f;
        float l = (0.2126f * mr + 0.7152f * mg) + 0.0722f * mb;
        if (!(l > 0.0f)) l = 0.0f;
        return sqrtf(v) / (l + 1e-2f);
    }
};

// Select: does list entry `pixel` stay active?  e and n are the state arrays of the whole image.
PTR_HD bool adaptiveKeep(uint32_t pixel, uint32_t width, uint32_t height, const float* e, const uint32_t* n, uint32_t maxSpp, float threshold) {
    const uint32_t x = pixel % width, y = pixel / width;
    const uint32_t y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < height ? y + 1u : height - 1u;
    const uint32_t x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < width ? x + 1u : width - 1u;
    float big = 0.0f;
    for (uint32_t qy = y0; qy <= y1; ++qy) {
        for (uint32_t qx = x0; qx <= x1; ++qx) {
            const float eq = e[static_cast<size_t>(qy) * width + qx];
            if (eq > big) big = eq;
        }
    }
    return n[pixel] < maxSpp && big > threshold;
}

#if defined(__HIPCC__)
// One sub-pass of a round: items[c * activeCount + j] is sample c of list entry j (rgb; w ignored), c < spp; the first is the frame's
// sample number nBefore (0-based).  The state of pixel list[j] is continued; n becomes nBefore + spp, and with `last` e is computed.
void launchAdaptiveUpdate(const float4* dItems, const uint32_t* dList, uint32_t activeCount, uint32_t spp, uint32_t nBefore, bool last,
                          const AdaptiveState& state, hipStream_t stream);
// Select + stable compaction: dNext receives the kept entries of dList in order, *dTotal their number.  dKeep: activeCount bytes;
// dBlockCounts / dBlockOffsets: ceil(activeCount / 256) words each.
struct AdaptiveScratch {
    uint8_t* keep;
    uint32_t* blockCounts;
    uint32_t* blockOffsets;
    uint32_t* total;
};
void launchAdaptiveSelect(const uint32_t* dList, uint32_t activeCount, uint32_t width, uint32_t height, const AdaptiveState& state, uint32_t maxSpp,
                          float threshold, const AdaptiveScratch& scratch, uint32_t* dNext, hipStream_t stream);
// The stable compaction alone (k_adaptive_scan, k_adaptive_scatter), for a caller that wrote the keep flags dKeep[activeCount] and the
// per-block counts scratch.blockCounts itself (frame.hip): dNext receives the kept entries of dList in order, *scratch.total their number.
void launchAdaptiveCompact(const uint32_t* dList, uint32_t activeCount, const uint8_t* dKeep, const AdaptiveScratch& scratch, uint32_t* dNext,
                           hipStream_t stream);
// rgb = sum / n, cov = M / (n (n - 1)), count = n for every pixel of the image (dCov and dCount may be null)
void launchAdaptiveFinish(const AdaptiveState& state, uint32_t pixels, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream);
#endif

#if defined(__HIP__)
// Device code of the compaction kernels (adaptive.hip, frame.hip), 256 threads per block.
constexpr uint32_t kCompactBlock = 256u;
constexpr uint32_t kCompactWaves = kCompactBlock / 64u;

// The rank of this thread's kept entry among the block's kept entries, and in blockTotal their number (every thread of the block calls).
__device__ inline uint32_t blockRank(bool keep, uint32_t* waveCounts, uint32_t& blockTotal) {
    const uint64_t votes = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) waveCounts[wave] = static_cast<uint32_t>(__popcll(votes));
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kCompactWaves; ++w) {
        const uint32_t cnt = waveCounts[w];
        if (w < wave) before += cnt;
        total += cnt;
    }
    blockTotal = total;
    return before + static_cast<uint32_t>(__popcll(votes & ((1ull << lane) - 1ull)));
}
#endif

}  // namespace ptrk
