// k_resolve_cov: the covariance of every pixel's mean from the frame's per-sample accumulators (include/ptr_stats.h, whose text this
// file follows line by line: float32, unfused - the Makefile compiles it with -ffp-contract=off - in the order written; so does the numpy
// restatement the tests compare it with, tests/stats_ref.py).
//
// One thread per local pixel, addressed like k_resolve: sample c of local pixel lp is item c * localPixels + lp, so a wave reads 1 KiB
// contiguous per sample, and a pass reads each of its accumulators once (Welford's recurrence is single-pass).  The loads do not depend
// on the recurrence: four are issued before the first is consumed.  A frame of several passes keeps the running mean in `mean` (one
// float4 per local pixel) and the unnormalised sums M in the output buffer between the passes.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace ptrk {

namespace {

constexpr uint32_t kCovUnroll = 4u;

struct Welford {
    float mr, mg, mb;
    float rr, gg, bb, rg, rb, gb;
    __device__ inline void add(const float4& x, uint32_t k) {
        const float fk = static_cast<float>(k);
        const float dr = x.x - mr, dg = x.y - mg, db = x.z - mb;
        mr = mr + dr / fk;
        mg = mg + dg / fk;
        mb = mb + db / fk;
        const float er = x.x - mr, eg = x.y - mg, eb = x.z - mb;
        rr += dr * er;
        gg += dg * eg;
        bb += db * eb;
        rg += dr * eg;
        rb += dr * eb;
        gb += dg * eb;
    }
};

__global__ void __launch_bounds__(256) k_resolve_cov(RenderParams rp, PathPool pool, uint32_t partCount, float4* mean, float* cov) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= rp.localPixels) return;
    const uint32_t pixel = pool.pixelOfLocal[lp];
    const uint32_t x = pixel % rp.width, y = pixel / rp.width;
    const uint32_t localBand = (y / PTR_BAND_ROWS) / partCount;
    float* o = cov + (static_cast<size_t>(localBand * PTR_BAND_ROWS + (y % PTR_BAND_ROWS)) * rp.width + x) * 6u;
    Welford w{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!(rp.passFlags & 1u)) {   // a later pass of the frame: go on from where the last one stopped
        const float4 m = mean[lp];
        w = Welford{m.x, m.y, m.z, o[0], o[1], o[2], o[3], o[4], o[5]};
    }
    const float4* items = pool.itemAccum + lp;
    const size_t stride = rp.localPixels;
    uint32_t c = 0;
    for (; c + kCovUnroll <= rp.spp; c += kCovUnroll) {
        float4 xs[kCovUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kCovUnroll; ++u) xs[u] = items[static_cast<size_t>(c + u) * stride];
#pragma unroll
        for (uint32_t u = 0; u < kCovUnroll; ++u) w.add(xs[u], rp.sampleBase + c + u + 1u);
    }
    for (; c < rp.spp; ++c) w.add(items[static_cast<size_t>(c) * stride], rp.sampleBase + c + 1u);
    if (rp.passFlags & 2u) {
        const float norm = static_cast<float>(rp.sppTotal) * static_cast<float>(rp.sppTotal - 1u);
        w.rr = w.rr / norm;
        w.gg = w.gg / norm;
        w.bb = w.bb / norm;
        w.rg = w.rg / norm;
        w.rb = w.rb / norm;
        w.gb = w.gb / norm;
    } else {
        mean[lp] = make_float4(w.mr, w.mg, w.mb, 0.0f);
    }
    o[0] = w.rr;
    o[1] = w.gg;
    o[2] = w.bb;
    o[3] = w.rg;
    o[4] = w.rb;
    o[5] = w.gb;
}

}  // namespace

void launchResolveCov(const RenderParams& rp, const PathPool& pool, uint32_t partCount, float4* dMean, float* dCov, hipStream_t stream) {
    hipLaunchKernelGGL(k_resolve_cov, dim3((rp.localPixels + 255u) / 256u), dim3(256), 0, stream, rp, pool, partCount, dMean, dCov);
}

}  // namespace ptrk
