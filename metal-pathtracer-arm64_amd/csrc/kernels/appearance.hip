// The kernels of include/ptr_appearance.h (launchers in appearance.h).  Compiled like dynamic.hip and rebuild.hip: unfused, with correctly
// rounded division, so every value is the upload's host arithmetic bit for bit.  What bounds each kernel:
// k_app_rekey        streams the triangle rows: per lane two 4 B loads 16 B apart out of a 48 B row (so every cache line of the array is
//                    fetched once), one byte gathered from a table of at most 64 KB that stays in cache, and a 4 B store only where the
//                    key differs.  Bandwidth bound on the reads.
// k_app_mip_level    one texel of the new level per lane: four 16 B loads (two adjacent pairs), one 16 B store, coalesced along x.
//                    Bandwidth bound; the small levels of a chain are launch bound (one launch per level, at most 15).
// k_app_env_weights  one row per lane, left to right, because the row sum's order is fixed: 16 B loads a row apart between lanes
//                    (uncoalesced: a 64 B line serves four steps of one lane), 4 B stores likewise.  A map has at most 4096 rows, so a
//                    few waves are in flight: latency bound, about `width` dependent loads long.
// k_app_env_total    ONE lane adds every weight in scan order - the order decides the bits of every pdf - while its workgroup (256
//                    lanes) stages the next 16 KB of weights through LDS, two buffers.  Bound by the dependent add and the LDS read it
//                    waits for, a few tens of cycles per texel; no other lane of the device does anything.  The kernel to look at
//                    when an environment update is slow.
// k_app_env_alias    one workgroup per table (a row's conditional table, or the marginal): the scaled values are written by all lanes,
//                    then one lane classifies them in index order and runs Vose's loop out of LDS (12 B per entry: 48 KB at the cap
//                    of 4096, three workgroups per CU), then all lanes write the tails.  Bound by the chain of dependent LDS accesses
//                    of that one lane; rows run side by side on as many CUs as there are rows.
// k_app_env_pdf      one texel per lane: 4 B in, 4 B out, two divisions.  Bandwidth bound.
// No kernel hands data between workgroups inside a launch; what one launch writes the next reads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "appearance.h"
#include "bvh_layout.h"

namespace ptrk {

namespace {

constexpr uint32_t kBlock = 256u;
constexpr uint32_t kTotalChunk = 4096u;   // floats per LDS buffer of k_app_env_total

uint32_t blocksFor(uint64_t n) { return static_cast<uint32_t>((n + kBlock - 1u) / kBlock); }

__global__ void __launch_bounds__(kBlock) k_app_rekey(float4* __restrict__ tris, uint32_t triCount, const uint8_t* __restrict__ keys, uint32_t materialCount,
                                                      uint32_t* __restrict__ changed) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool wrote = false;
    if (t < triCount) {
        uint32_t* words = reinterpret_cast<uint32_t*>(tris + static_cast<size_t>(t) * 3u);
        const uint32_t material = words[3];
        const uint32_t meta = words[7];
        const uint32_t key = keys[material < materialCount ? material : materialCount - 1u];
        const uint32_t next = (meta & ~(kHitKeyMask << kHitKeyShift)) | ((key & kHitKeyMask) << kHitKeyShift);
        // (a row that was never keyed - the zero rows a dynamic scene's object-space corners hold for rectangle halves - stays as it is)
        if (next != meta && ((meta >> kHitKeyShift) & kHitKeyMask) != 0u) {
            words[7] = next;
            wrote = true;
        }
    }
    const unsigned long long votes = __ballot(wrote);
    if ((threadIdx.x & 63u) == 0u && votes != 0ull) atomicAdd(changed, static_cast<uint32_t>(__popcll(votes)));
}

__global__ void __launch_bounds__(kBlock) k_app_mip_level(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t w, uint32_t h, uint32_t nw,
                                                          uint32_t nh) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= static_cast<size_t>(nw) * nh) return;
    const uint32_t y = static_cast<uint32_t>(i / nw), x = static_cast<uint32_t>(i - static_cast<size_t>(y) * nw);
    const uint32_t y0 = min(2u * y, h - 1u), y1 = min(2u * y + 1u, h - 1u);
    const uint32_t x0 = min(2u * x, w - 1u), x1 = min(2u * x + 1u, w - 1u);
    const float4 a = src[static_cast<size_t>(y0) * w + x0], b = src[static_cast<size_t>(y0) * w + x1];
    const float4 c = src[static_cast<size_t>(y1) * w + x0], d = src[static_cast<size_t>(y1) * w + x1];
    float4 o;
    o.x = ((a.x + b.x) + (c.x + d.x)) * 0.25f;
    o.y = ((a.y + b.y) + (c.y + d.y)) * 0.25f;
    o.z = ((a.z + b.z) + (c.z + d.z)) * 0.25f;
    o.w = ((a.w + b.w) + (c.w + d.w)) * 0.25f;
    dst[i] = o;
}

__global__ void __launch_bounds__(kBlock) k_app_env_weights(const float4* __restrict__ rgba, const float* __restrict__ cell, uint32_t width, uint32_t height,
                                                            float* __restrict__ weight, float* __restrict__ rowWeight) {
    const uint32_t y = blockIdx.x * kBlock + threadIdx.x;
    if (y >= height) return;
    const float c = cell[y];
    const float4* px = rgba + static_cast<size_t>(y) * width;
    float* w = weight + static_cast<size_t>(y) * width;
    float sum = 0.0f;
    for (uint32_t x = 0; x < width; ++x) {
        const float4 p = px[x];
        const float lum = (0.2126f * p.x + 0.7152f * p.y) + 0.0722f * p.z;
        const float v = (lum < 0.0f ? 0.0f : lum) * c;   // std::max(lum, 0.0f)
        w[x] = v;
        sum += v;
    }
    rowWeight[y] = sum;
}

__global__ void __launch_bounds__(kBlock) k_app_env_total(const float* __restrict__ weight, uint64_t count, float* __restrict__ total) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* buf = reinterpret_cast<float*>(smem);   // two buffers of kTotalChunk floats
    const uint64_t chunks = (count + kTotalChunk - 1u) / kTotalChunk;
    auto stage = [&](uint64_t chunk, float* into) {
        const uint64_t base = chunk * kTotalChunk;
        for (uint32_t k = threadIdx.x; k < kTotalChunk; k += kBlock) into[k] = base + k < count ? weight[base + k] : 0.0f;
    };
    if (chunks > 0u) stage(0u, buf);
    __syncthreads();
    float sum = 0.0f;
    for (uint64_t c = 0; c < chunks; ++c) {
        float* cur = buf + (c & 1u) * kTotalChunk;
        if (c + 1u < chunks) stage(c + 1u, buf + ((c + 1u) & 1u) * kTotalChunk);
        if (threadIdx.x == 0u) {
            const uint64_t base = c * kTotalChunk;
            const uint32_t n = static_cast<uint32_t>(count - base < kTotalChunk ? count - base : kTotalChunk);
            for (uint32_t k = 0; k < n; ++k) sum += cur[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0u) total[0] = sum;
}

// Vose's alias method as ptr::BuildEnvImportanceDistribution's buildAlias runs it, on the table of block b: a row's conditional table
// (b < height) or the marginal (b == height).
__global__ void __launch_bounds__(kBlock) k_app_env_alias(const float* __restrict__ weight, const float* __restrict__ rowWeight, const float* __restrict__ totalPtr,
                                                          uint32_t width, uint32_t height, float2* __restrict__ cond, float2* __restrict__ marg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool marginal = blockIdx.x == height;
    const uint32_t count = marginal ? height : width;
    float* scaled = reinterpret_cast<float*>(smem);
    uint32_t* under = reinterpret_cast<uint32_t*>(smem) + count;
    uint32_t* over = under + count;
    uint32_t* tails = over + count;   // the lengths the two lists end with (everything in the dynamic region: its base stays 16 B aligned)
    float2* out = marginal ? marg : cond + static_cast<size_t>(blockIdx.x) * width;
    const float total = totalPtr[0];
    const float fcount = static_cast<float>(count);
    if (marginal) {
        for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
            const float rw = rowWeight[i];
            const float prob = rw > 0.0f ? rw / total : 0.0f;
            scaled[i] = prob * fcount;
        }
    } else {
        const float rw = rowWeight[blockIdx.x];
        const float* w = weight + static_cast<size_t>(blockIdx.x) * width;
        const float inv = 1.0f / rw;
        const float uniform = 1.0f / static_cast<float>(width);
        for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
            const float prob = rw > 0.0f ? w[i] * inv : uniform;
            scaled[i] = prob * fcount;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t nu = 0u, no = 0u;
        for (uint32_t i = 0; i < count; ++i) {
            if (scaled[i] < 1.0f) under[nu++] = i;
            else over[no++] = i;
        }
        while (nu > 0u && no > 0u) {
            const uint32_t u = under[--nu];
            const uint32_t o = over[no - 1u];
            const float su = scaled[u];
            const float lo = su < 0.0f ? 0.0f : su;        // std::max(scaled[u], 0.0f)
            out[u] = make_float2(1.0f < lo ? 1.0f : lo, __uint_as_float(o));   // std::min(.., 1.0f)
            const float so = (scaled[o] + su) - 1.0f;
            scaled[o] = so;
            if (so < 1.0f - 1e-7f) {
                --no;
                under[nu++] = o;
            }
        }
        tails[0] = nu, tails[1] = no;
    }
    __syncthreads();
    const uint32_t nu = tails[0], no = tails[1];
    for (uint32_t k = threadIdx.x; k < nu; k += kBlock) out[under[k]] = make_float2(1.0f, __uint_as_float(under[k]));
    for (uint32_t k = threadIdx.x; k < no; k += kBlock) out[over[k]] = make_float2(1.0f, __uint_as_float(over[k]));
}

__global__ void __launch_bounds__(kBlock) k_app_env_pdf(const float* __restrict__ weight, const float* __restrict__ cell, const float* __restrict__ totalPtr,
                                                        uint32_t width, uint64_t count, float* __restrict__ pdf) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= count) return;
    const float c = cell[i / width];
    pdf[i] = c > 0.0f ? (weight[i] / totalPtr[0]) / c : 0.0f;
}

}  // namespace

void launchAppRekey(float4* dTris, uint32_t triCount, const uint8_t* dKeys, uint32_t materialCount, uint32_t* dChanged, hipStream_t stream) {
    if (triCount > 0u && materialCount > 0u) {
        hipLaunchKernelGGL(k_app_rekey, dim3(blocksFor(triCount)), dim3(kBlock), 0, stream, dTris, triCount, dKeys, materialCount, dChanged);
    }
}

void launchAppMipLevel(const float4* dSrc, float4* dDst, uint32_t w, uint32_t h, uint32_t nw, uint32_t nh, hipStream_t stream) {
    const uint64_t n = static_cast<uint64_t>(nw) * nh;
    if (n > 0u && w > 0u && h > 0u) hipLaunchKernelGGL(k_app_mip_level, dim3(blocksFor(n)), dim3(kBlock), 0, stream, dSrc, dDst, w, h, nw, nh);
}

void launchAppEnvWeights(const float4* dRgba, const float* dCell, uint32_t width, uint32_t height, float* dWeight, float* dRowWeight, hipStream_t stream) {
    if (width > 0u && height > 0u) {
        hipLaunchKernelGGL(k_app_env_weights, dim3(blocksFor(height)), dim3(kBlock), 0, stream, dRgba, dCell, width, height, dWeight, dRowWeight);
    }
}

void launchAppEnvTotal(const float* dWeight, uint64_t count, float* dTotal, hipStream_t stream) {
    hipLaunchKernelGGL(k_app_env_total, dim3(1), dim3(kBlock), 2u * kTotalChunk * sizeof(float), stream, dWeight, count, dTotal);
}

void launchAppEnvAlias(const float* dWeight, const float* dRowWeight, const float* dTotal, uint32_t width, uint32_t height, float2* dCond, float2* dMarg,
                       hipStream_t stream) {
    const uint32_t entries = std::max(width, height);
    if (width == 0u || height == 0u || entries > kAppAliasMaxEntries) return;   // (the entry points refuse such a map)
    hipLaunchKernelGGL(k_app_env_alias, dim3(height + 1u), dim3(kBlock), static_cast<size_t>(entries) * 12u + 16u, stream, dWeight, dRowWeight, dTotal, width, height,
                       dCond, dMarg);
}

void launchAppEnvPdf(const float* dWeight, const float* dCell, const float* dTotal, uint32_t width, uint32_t height, float* dPdf, hipStream_t stream) {
    const uint64_t n = static_cast<uint64_t>(width) * height;
    if (n > 0u) hipLaunchKernelGGL(k_app_env_pdf, dim3(blocksFor(n)), dim3(kBlock), 0, stream, dWeight, dCell, dTotal, width, n, dPdf);
}

}  // namespace ptrk
